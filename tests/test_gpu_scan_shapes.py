"""
The int64 exclusive scan (`exclusive_scan_i64`, cip_plan.hip) at the sizes where its shape changes: one-wave
blocks of 4096 items in 16 rounds of 256 (4 consecutive items per lane), recursion over the block sums.

Path: `cip_tile_runs` scans its per-row run counts directly (`row_runs`, nrow + 1 items) and writes run k of
row r at the scanned offset, so the emitted row column IS the scan: with one channel every row is exactly one
run, the offsets are arange(nrow + 1), the total is nrow and run k belongs to row k. The sizes are
n = nrow + 1 around one lane's items, one round, one block, two blocks and the first size with three scan
levels (4096^2 + 1). `cip_tile_runs` has no rows without a run (every row has a key for its first channel),
so the mixed case mixes rows of one and of two runs instead: two channels whose keys differ for some rows.
Exact equality throughout.
"""

import ctypes

import pytest

from ska_sdp_cip_amd._call import STREAM, call

pytestmark = pytest.mark.gpu

SPEED_OF_LIGHT = 299792458.0
SIZES = [1, 2, 63, 64, 65, 4095, 4096, 4097, 8193, 4096 ** 2 - 1, 4096 ** 2, 4096 ** 2 + 1]


def _tile_runs(torch, uvw, freqs, tile):
    """(total, run rows (device int64), run channel starts) of cip_tile_runs on device tensors."""
    dev = uvw.device
    nrow = int(uvw.shape[0])
    ts = (ctypes.c_double * 3)(*tile)
    n = ctypes.c_int64(0)
    args = (uvw, nrow, freqs, int(freqs.numel()), ts, 0, STREAM, ctypes.byref(n))
    call(dev, "cip_tile_runs", *args, None, None, None, None)
    total = n.value
    key = torch.empty((max(total, 1), 3), dtype=torch.int64, device=dev)
    row = torch.empty(max(total, 1), dtype=torch.int64, device=dev)
    c0 = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
    c1 = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
    if total:
        call(dev, "cip_tile_runs", *args, key, row, c0, c1)
    return total, row[:total], c0[:total]


@pytest.mark.parametrize("n", SIZES)
def test_scan_of_ones_is_arange(gpu_device, n):
    import torch

    nrow = n - 1
    gen = torch.Generator(device=gpu_device).manual_seed(n)
    uvw = torch.rand((nrow, 3), dtype=torch.float64, device=gpu_device, generator=gen) * 1000.0
    freqs = torch.tensor([1.0e9], dtype=torch.float64, device=gpu_device)
    total, row, c0 = _tile_runs(torch, uvw, freqs, (100.0, 100.0, 100.0))
    assert total == nrow
    if nrow:
        assert torch.equal(row, torch.arange(nrow, dtype=torch.int64, device=gpu_device))
        assert not bool(c0.any())


@pytest.mark.parametrize("n", [65, 4097, 3 * 4096 + 18])
def test_scan_of_mixed_counts(gpu_device, n):
    import torch

    # frequencies c and 2 c: the keys are floor(u + 0.5) and floor(2 u + 0.5) (tile size 1, exact in fp64):
    # u = 0 gives one run (keys 0, 0), u = 3 two (keys 3, 6)
    nrow = n - 1
    gen = torch.Generator(device=gpu_device).manual_seed(1000 + n)
    two = torch.rand(nrow, device=gpu_device, generator=gen) < 0.4
    uvw = torch.zeros((nrow, 3), dtype=torch.float64, device=gpu_device)
    uvw[:, 0] = torch.where(two, 3.0, 0.0).to(torch.float64)
    freqs = torch.tensor([SPEED_OF_LIGHT, 2.0 * SPEED_OF_LIGHT], dtype=torch.float64, device=gpu_device)
    counts = 1 + two.to(torch.int64)
    total, row, c0 = _tile_runs(torch, uvw, freqs, (1.0, 1.0, 1.0))
    assert total == int(counts.sum())
    rows = torch.arange(nrow, dtype=torch.int64, device=gpu_device)
    assert torch.equal(row, torch.repeat_interleave(rows, counts))
    # a row's second run starts at channel 1, right after its first
    second = torch.zeros(total, dtype=torch.bool, device=gpu_device)
    second[1:] = row[1:] == row[:-1]
    assert torch.equal(c0.to(torch.int64), second.to(torch.int64))
