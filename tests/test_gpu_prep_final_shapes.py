"""
The final weight-sum reduction (`prep_final_kernel`, cip_grid.hip) at the place-block counts where its order
changes shape, and the order itself.

The order is part of the result (the weight sum normalises the image): place block b (4096 visibilities)
reduces its weights to one fp64 partial, and the final reduction adds the partials in the order of a block of
1024 threads - thread t sums the partials t + 1024 k + 4096 j into accumulator k (j ascending), combines the
accumulators as (0 + 1) + (2 + 3), a 64-lane xor-shuffle tree (d = 32 .. 1) gives each of the 16 waves its
total, and the wave totals are added in wave order. One wave computes that order; the block counts 1, 2, 1023,
1024, 1025, 4096 and 4097 straddle the 1024-thread and the 4 x 1024 strides.

Exact case: weights from {0, 0.5, 1, 1.5} and visibility parts that are multiples of 1/4 of magnitude <= 1,
so every fp64 sum is exact in any order - the returned sum must be THE sum, and the pipelined call's image
must equal the synchronous call's bit for bit. Order case: random float32 weights at 1025 blocks against a
numpy restatement of the place pass's per-block partials and of the order above, bit for bit.
"""

import numpy as np
import pytest

from ska_sdp_cip_amd import gridder

pytestmark = pytest.mark.gpu

NCHAN = 64  # dense rows of a multiple of 64 channels: the benchmark's place pass
BLOCK_VIS = 4096
NPIX = 128
C = 299792458.0


def _inputs(torch, dev, nblocks, seed, exact):
    nrow = nblocks * BLOCK_VIS // NCHAN
    gen = torch.Generator(device=dev).manual_seed(seed)
    # |u|, |v| up to 400 wavelengths at the top channel; the uv plane of the image spans 1 / px = 1040 of them
    uvw = (torch.rand((nrow, 3), dtype=torch.float64, device=dev, generator=gen) - 0.5) * 800.0
    uvw[:, 2] = 0.0
    freq = torch.linspace(0.9, 1.0, NCHAN, dtype=torch.float64, device=dev) * C  # wavelengths 1.0 .. 1.11 m
    px = 1.0 / (2 * 400.0 * 1.3)
    if exact:
        wgt = torch.randint(0, 4, (nrow, NCHAN), device=dev, generator=gen).to(torch.float32) * 0.5
        re = torch.randint(-2, 3, (nrow, NCHAN), device=dev, generator=gen).to(torch.float32) * 0.25
        im = torch.randint(-2, 3, (nrow, NCHAN), device=dev, generator=gen).to(torch.float32) * 0.25
    else:
        wgt = torch.rand((nrow, NCHAN), dtype=torch.float32, device=dev, generator=gen)
        re = torch.rand((nrow, NCHAN), dtype=torch.float32, device=dev, generator=gen) - 0.5
        im = torch.rand((nrow, NCHAN), dtype=torch.float32, device=dev, generator=gen) - 0.5
    return uvw, freq, torch.complex(re, im).contiguous(), wgt.contiguous(), px


def _invert(torch, dev, inputs, **kw):
    uvw, freq, vis, wgt, px = inputs
    sumw = torch.zeros(1, dtype=torch.float64, device=dev)
    out, _ = gridder.device_ms2dirty(uvw, freq, vis, wgt, NPIX, NPIX, px, px, support=8, sum_weights=sumw, **kw)
    return out, sumw


@pytest.mark.parametrize("nblocks", [1, 2, 1023, 1024, 1025, 4096, 4097])
def test_exact_weight_sum_and_pipelined_image(gpu_device, nblocks):
    import torch

    inputs = _inputs(torch, gpu_device, nblocks, 100 + nblocks, exact=True)
    exact = float(inputs[3].to(torch.float64).sum().item())  # multiples of 0.5 below 2^53: exact in any order
    img_sync, sw_sync = _invert(torch, gpu_device, inputs)
    assert float(sw_sync.item()) == exact
    # the pipelined form: an asynchronous call, then one whose planner runs beside it
    _invert(torch, gpu_device, inputs, synchronize=False)
    img_pipe, sw_pipe = _invert(torch, gpu_device, inputs, synchronize=False, resident_inputs=True)
    torch.cuda.synchronize()
    assert float(sw_pipe.item()) == exact
    assert torch.equal(img_pipe, img_sync)


def _tree(x):
    """The 64-lane xor-shuffle tree over the last axis (every lane ends with the total in lane 0's order)."""
    lanes = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        x = x + x[..., lanes ^ d]
    return x


def _ordered_sum(wgt):
    """The weight sum in the library's order: place-block partials, then the final reduction."""
    w = wgt.astype(np.float64).reshape(-1, 16, 4, 64)  # (block, step, wave, lane): wave w takes every 4th segment
    acc = np.zeros((w.shape[0], 4, 64))
    for it in range(16):
        acc = acc + w[:, it]
    ss = _tree(acc)[..., 0]  # (block, wave)
    partial = (ss[:, 0] + ss[:, 1]) + (ss[:, 2] + ss[:, 3])
    # thread t of 1024: accumulator k sums the partials t + 1024 k + 4096 j, j ascending
    pad = np.zeros(-(-partial.size // 4096) * 4096)
    pad[:partial.size] = partial  # (adding the 0.0 of a missing partial changes no sum of non-negative terms)
    p = pad.reshape(-1, 4, 1024)
    acc = np.zeros((4, 1024))
    for j in range(p.shape[0]):
        acc = acc + p[j]
    s = ((acc[0] + acc[1]) + (acc[2] + acc[3])).reshape(16, 64)
    totals = _tree(s)[:, 0]
    t = 0.0
    for wv in range(16):
        t = t + float(totals[wv])
    return t


def test_weight_sum_order_at_1025_blocks(gpu_device):
    import torch

    inputs = _inputs(torch, gpu_device, 1025, 7, exact=False)
    _, sumw = _invert(torch, gpu_device, inputs)
    want = _ordered_sum(inputs[3].cpu().numpy())
    got = float(sumw.item())
    print(f"sum of weights: library {got!r}, restated order {want!r}")
    assert got == want
