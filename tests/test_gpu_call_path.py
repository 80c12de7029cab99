"""
The call path into the library (`_call.call`): a call on tensors of a device
that is not current runs on their device and leaves the current device alone,
tensors on different devices are refused before the library is reached, and
the strip split of a strip no footprint starts in returns empty members
without an emit pass.
"""
import numpy as np
import pytest
import torch

from ska_sdp_cip_amd import _lib, gridder, strips
from ska_sdp_cip_amd import synthetic as syn

pytestmark = pytest.mark.gpu


def _two_gpus():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    return torch.device("cuda", 0), torch.device("cuda", 1)


def test_call_on_a_device_that_is_not_current(gpu_device):
    dev0, dev1 = _two_gpus()
    ms = syn.make_measurement_set(64, 4, n_ant=12, array_radius_m=800.0, seed=3)
    uvw, f = torch.from_numpy(ms.uvw()), torch.from_numpy(ms.channel_frequencies())
    px = syn.pixel_size_for_grid(ms.uvw(), ms.channel_frequencies(), 256)
    prm = _lib.choose_params(256, 256, px, px, 1e-4, 8)
    with torch.cuda.device(dev0):
        want = strips.strip_histogram(uvw.to(dev0), f.to(dev0), prm, px, px)
        got = strips.strip_histogram(uvw.to(dev1), f.to(dev1), prm, px, px)
        assert torch.cuda.current_device() == 0
    assert int(want[0].sum()) == 64 * 4
    for a, b in zip(want, got):
        assert b.device == dev1 and torch.equal(a.cpu(), b.cpu())


def test_tensors_on_different_devices_are_refused(gpu_device, monkeypatch):
    dev0, dev1 = _two_gpus()

    def no_call(*args):
        raise AssertionError(f"the library was reached: {args[1]}")

    monkeypatch.setattr(gridder, "call", no_call)
    vis4 = torch.zeros((8, 4, 4), dtype=torch.complex64, device=dev0)
    flags4 = torch.zeros((8, 4, 4), dtype=torch.uint8, device=dev0)
    wgt4 = torch.ones((8, 4, 4), dtype=torch.float32, device=dev1)
    with pytest.raises(ValueError):
        gridder.device_stokes(vis4, flags4, wgt4)
    with pytest.raises(ValueError):
        gridder.device_stokes_i(vis4, flags4, wgt4)
    uvw = torch.zeros((8, 3), dtype=torch.float64, device=dev0)
    with pytest.raises(ValueError):
        gridder.device_facet_rephase(uvw, torch.ones(4, dtype=torch.float64, device=dev1), None, 0.0, 0.0)


def test_empty_strip_is_split_without_an_emit_pass(gpu_device):
    nrow, nchan = 8, 4
    uvw = np.zeros((nrow, 3))
    uvw[:, 0] = np.linspace(-200.0, 200.0, nrow)  # v = 0: every footprint origin lies near row nv / 2
    f = np.linspace(1.0e9, 1.1e9, nchan)
    px = syn.pixel_size_for_grid(uvw, f, 256)
    prm = _lib.choose_params(256, 256, px, px, 1e-4, 8)
    du, df = torch.from_numpy(uvw).to(gpu_device), torch.from_numpy(f).to(gpu_device)
    dv = torch.ones((nrow, nchan), dtype=torch.complex64, device=gpu_device)
    dw = torch.ones((nrow, nchan), dtype=torch.float64, device=gpu_device)
    full = strips.split_strip(du, df, dv, dw, prm, px, 0, prm.nv)
    assert full.nvis == nrow * nchan and full.slice_uvw.shape == (nrow, 3)
    assert int(full.rows.min()) == 0 and int(full.rows.max()) == nrow - 1
    empty = strips.split_strip(du, df, dv, dw, prm, px, 0, int(prm.support))
    members = (empty.slice_uvw, empty.chan_start, empty.chan_stop, empty.vis, empty.wgt, empty.rows)
    assert [int(m.shape[0]) for m in members] == [0] * 6 and empty.slice_uvw.shape == (0, 3)
    for got, ref in zip(members, (full.slice_uvw, full.chan_start, full.chan_stop, full.vis, full.wgt, full.rows)):
        assert got.dtype == ref.dtype and got.device == ref.device
    assert (empty.chan_start.dtype, empty.rows.dtype) == (torch.int32, torch.int64)
    assert (empty.vis.dtype, empty.wgt.dtype) == (dv.dtype, dw.dtype)
    rows, c0, c1 = strips.strip_slices(du, df, prm, px, 0, int(prm.support))
    assert rows.numel() == c0.numel() == c1.numel() == 0 and c0.dtype == torch.int64
