"""
Host-side checks of the gain calibration (no GPU): include/cip_cal.h against
`_lib.CAL_PROTOTYPES` and the struct mirrors (the method of test_mfs_host.py on
the fourth header), the hand values of `cip_cal_scale_init`, every CIP_EINVAL
refused before the device, `solution_intervals` and `baseline_indices`, and the
numpy statement `_cal_np` on noise-free data.
"""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import _cal_np
from ska_sdp_cip_amd import _lib, calibrate, synthetic

HEADER = Path(__file__).resolve().parents[1] / "include" / "cip_cal.h"
SCALARS = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "int": ctypes.c_int, "double": ctypes.c_double}
STRUCTS = {"cip_cal_scale": _lib.CalScale, "cip_cal_counts": _lib.CalCounts,
           "cip_cal_solve_info": _lib.CalSolveInfo}
NAMES = ("cip_cal_scale_init", "cip_cal_correlate", "cip_cal_solve", "cip_cal_apply", "cip_gaincal")


@pytest.fixture(scope="module")
def header():
    text = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


# ---- header against table ----------------------------------------------------
def test_every_prototype_matches_the_table(header):
    protos = {}
    for ret, name, params in re.findall(r"\b(int|const\s+char\s*\*)\s*(cip_\w+)\s*\(([^)]*)\)\s*;", header):
        protos[name] = (ret, [" ".join(p.split()) for p in params.split(",")])
    assert tuple(protos) == tuple(_lib.CAL_PROTOTYPES) == NAMES
    for name, (ret, params) in protos.items():
        restype, argtypes = _lib.CAL_PROTOTYPES[name]
        assert ret == "int" and restype is ctypes.c_int, name
        assert len(argtypes) == len(params), (name, len(argtypes), len(params))
        for k, (decl, argtype) in enumerate(zip(params, argtypes)):
            if "*" in decl:
                base = decl.replace("const", " ").split("*")[0].strip()
                if base in STRUCTS:  # the structs are host memory
                    assert argtype is ctypes.POINTER(STRUCTS[base]), (name, k, decl)
                else:
                    assert argtype is ctypes.c_void_p, (name, k, decl)
            else:
                assert argtype is SCALARS[decl.replace("const", " ").split()[0]], (name, k, decl)
    assert '#include "cip.h"' in header and 'extern "C"' in header


def test_struct_mirrors_and_defines_match_the_header(header):
    structs = dict(re.findall(r"typedef\s+struct\s+(cip_\w+)\s*\{(.*?)\}\s*\1\s*;", header, flags=re.S))
    assert set(structs) == set(STRUCTS)
    for name, mirror in STRUCTS.items():
        fields = []
        for decl in filter(None, (" ".join(d.split()) for d in structs[name].split(";"))):
            ctype, names = decl.split(" ", 1)
            fields += [(n.strip(), SCALARS[ctype]) for n in names.split(",")]
        assert fields == list(mirror._fields_), name  # pylint: disable=protected-access
    sizes = [ctypes.sizeof(STRUCTS[n]) for n in ("cip_cal_scale", "cip_cal_counts", "cip_cal_solve_info")]
    assert sizes == [48, 32, 40]
    defines = {k: int(v) for k, v in re.findall(r"#define\s+(CIP_\w+)\s+(\d+)", header)}
    assert defines == {"CIP_CAL_MAX_ANT": 1024, "CIP_CAL_CORRECT": 0, "CIP_CAL_CORRUPT": 1, "CIP_CAL_PHASE_ONLY": 1}
    assert (_lib.CAL_MAX_ANT, _lib.CAL_CORRECT, _lib.CAL_CORRUPT, _lib.CAL_PHASE_ONLY) == (1024, 0, 1, 1)
    assert _lib.CAL_MODES == {"correct": 0, "corrupt": 1} and _cal_np.MAX_ANT == 1024


def test_library_exports_and_other_tables_unchanged():
    so = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in _lib.CAL_PROTOTYPES:
        assert hasattr(so, name), name
        assert name not in _lib.PROTOTYPES and name not in _lib.RESTORE_PROTOTYPES and name not in _lib.MFS_PROTOTYPES
    assert (len(_lib.PROTOTYPES), len(_lib.RESTORE_PROTOTYPES), len(_lib.MFS_PROTOTYPES)) == (41, 6, 1)
    assert _lib.EXPORTED_SYMBOLS == tuple(_lib.PROTOTYPES)
    loaded = _lib.lib()  # lib() applies all four tables
    for name, (restype, argtypes) in _lib.CAL_PROTOTYPES.items():
        fn = getattr(loaded, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


# ---- cip_cal_scale_init -------------------------------------------------------
@pytest.mark.parametrize("amax, wmax, nsamp, shift", [
    (1.0, 1.0, 1, 59),            # B = 0; x = 2 < 2^2: E = 2
    (1.0, 1.0, 2, 58),            # 2 <= 2^1
    (1.0, 1.0, 3, 57),            # 3 <= 2^2
    (1.0, 1.0, 1024, 49),         # B = 10
    (1.0, 1.0, 1025, 48),
    (3.0, 0.5, 1, 57),            # x = 9 < 2^4
    (0.5, 1.0, 1, 61),            # x = 0.5 < 2^0: E = 0
    (1.0, 0.4999, 1, 61),         # x just below 1
    (1.5, 1.5, 100_000_000, 31),  # x = 6.75 < 2^3, B = 27
    (1e3, 1e-2, 1, 46),           # x = 2e4 < 2^15
])
def test_scale_init_hand_values(amax, wmax, nsamp, shift):
    s = _lib.cal_scale(8, 2, amax, wmax, nsamp)
    assert (s.n_ant, s.n_int, s.amax, s.wmax, s.reserved) == (8, 2, amax, wmax, 0)
    assert s.shift == shift and s.quantum == 2.0 ** -shift
    assert s.corr_shape == (2, 8, 8, 3)
    ref = _cal_np.scale_init(8, 2, amax, wmax, nsamp)
    assert (ref["shift"], ref["quantum"]) == (s.shift, s.quantum)
    # no sum of nsamp terms of magnitude <= 2 wmax amax^2 reaches 2^62
    assert nsamp * (2.0 * wmax * amax * amax) * 2.0 ** shift < 2.0 ** 62


def test_scale_init_refusals():
    so, out = _lib.lib(), _lib.CalScale()

    def call(n_ant=8, n_int=2, amax=1.0, wmax=1.0, nsamp=10, ptr=ctypes.byref(out)):
        return so.cip_cal_scale_init(n_ant, n_int, amax, wmax, nsamp, ptr)

    assert call() == _lib.CIP_OK
    nan, inf = float("nan"), float("inf")
    for kw in (dict(amax=0.0), dict(amax=-1.0), dict(amax=nan), dict(amax=inf), dict(wmax=0.0), dict(wmax=-2.0),
               dict(wmax=nan), dict(wmax=inf), dict(nsamp=0), dict(nsamp=-5), dict(n_ant=1), dict(n_ant=0),
               dict(n_ant=1025), dict(n_int=0), dict(n_int=-1), dict(ptr=None), dict(amax=1e200, wmax=1e200)):
        assert call(**kw) == _lib.CIP_EINVAL, kw
        assert b"cip_cal_scale_init" in so.cip_last_error(), kw
    assert call(n_ant=2) == _lib.CIP_OK and call(n_ant=1024) == _lib.CIP_OK
    with pytest.raises(ValueError, match="n_ant"):
        _lib.cal_scale(1, 1, 1.0, 1.0, 1)


# ---- every CIP_EINVAL comes before the device -----------------------------------
def test_argument_checks_come_before_the_device():
    so = _lib.lib()
    fake = [ctypes.c_void_p(4096 * k) for k in range(1, 10)]  # never dereferenced: every call below is refused
    scale = _lib.cal_scale(8, 2, 1.0, 1.0, 100)
    broken = _lib.CalScale()  # zeros: not filled by cip_cal_scale_init
    counts, info = _lib.CalCounts(), _lib.CalSolveInfo()
    c64, c128, f32, f64, none = _lib.CIP_C64, _lib.CIP_C128, _lib.CIP_F32, _lib.CIP_F64, _lib.CIP_NONE
    nan, inf = float("nan"), float("inf")

    def correlate(vis=fake[0], vd=c64, model=fake[1], md=c128, wgt=fake[2], wd=f32, nrow=4, nchan=3, a1=fake[3],
                  a2=fake[4], iv=fake[5], sc=scale, corr=fake[6]):
        return so.cip_cal_correlate(vis, vd, model, md, wgt, wd, nrow, nchan, a1, a2, iv,
                                    None if sc is None else ctypes.byref(sc), None, corr, ctypes.byref(counts))

    for kw in (dict(vd=f32), dict(md=0), dict(wd=none), dict(wd=c64), dict(nrow=-1), dict(nchan=0), dict(nchan=65536),
               dict(vis=None), dict(model=None), dict(wgt=None), dict(a1=None), dict(a2=None), dict(iv=None),
               dict(sc=None), dict(sc=broken), dict(corr=None)):
        assert correlate(**kw) == _lib.CIP_EINVAL, kw
        assert b"cip_cal_correlate" in so.cip_last_error(), kw

    def solve(corr=fake[0], sc=scale, niter=5, tol=1e-8, refant=0, flags=0, gains=fake[1], ok=fake[2]):
        return so.cip_cal_solve(corr, None if sc is None else ctypes.byref(sc), niter, tol, refant, flags, None,
                                gains, ok, None, ctypes.byref(info))

    for kw in (dict(niter=-1), dict(tol=-1e-9), dict(tol=nan), dict(tol=inf), dict(refant=8), dict(refant=100),
               dict(flags=2), dict(sc=None), dict(sc=broken), dict(corr=None), dict(gains=None), dict(ok=None)):
        assert solve(**kw) == _lib.CIP_EINVAL, kw
        assert b"cip_cal_solve" in so.cip_last_error(), kw

    def apply(vis=fake[0], vd=c64, wgt=fake[1], wd=f32, nrow=4, nchan=3, a1=fake[2], a2=fake[3], iv=fake[4],
              gains=fake[5], ok=fake[6], n_int=2, n_ant=8, mode=0, out=fake[7], wout=fake[8]):
        return so.cip_cal_apply(vis, vd, wgt, wd, nrow, nchan, a1, a2, iv, gains, ok, n_int, n_ant, mode, None, out,
                                wout)

    for kw in (dict(vd=f64), dict(wd=c64), dict(wgt=None), dict(wout=None), dict(wgt=None, wout=None),
               dict(wd=none), dict(nrow=-1), dict(nchan=0), dict(a1=None), dict(iv=None), dict(gains=None),
               dict(ok=None), dict(n_int=0), dict(n_ant=1), dict(n_ant=1025), dict(mode=2), dict(mode=-1),
               dict(vis=None), dict(out=None)):
        assert apply(**kw) == _lib.CIP_EINVAL, kw
        assert b"cip_cal_apply" in so.cip_last_error(), kw

    def gaincal(vis=fake[0], vd=c64, model=fake[1], md=c64, wgt=fake[2], wd=f64, nrow=4, nchan=3, a1=fake[3],
                a2=fake[4], iv=fake[5], n_ant=8, n_int=2, niter=5, tol=1e-8, refant=0, flags=1, gains=fake[6],
                ok=fake[7]):
        return so.cip_gaincal(vis, vd, model, md, wgt, wd, nrow, nchan, a1, a2, iv, n_ant, n_int, niter, tol, refant,
                              flags, None, gains, ok, None, None, None, None)

    for kw in (dict(vd=f32), dict(md=none), dict(wd=none), dict(nrow=-1), dict(nchan=0), dict(vis=None),
               dict(model=None), dict(wgt=None), dict(a2=None), dict(n_ant=1), dict(n_ant=1025), dict(n_int=0),
               dict(niter=-1), dict(tol=-1.0), dict(tol=nan), dict(refant=8), dict(flags=4), dict(gains=None),
               dict(ok=None)):
        assert gaincal(**kw) == _lib.CIP_EINVAL, kw
        assert b"cip_" in so.cip_last_error(), kw


# ---- solution_intervals, baseline_indices, random_gains ----------------------------
def test_solution_intervals():
    t = np.array([0, 0, 1, 7, 8, 15, 16, 17], dtype=np.int32)
    out = calibrate.solution_intervals(t, 8)
    assert out.dtype == np.int32 and out.tolist() == [0, 0, 0, 0, 1, 1, 2, 2]
    assert calibrate.solution_intervals(t, 1).tolist() == t.tolist()
    assert calibrate.solution_intervals(t, 100).tolist() == [0] * 8
    import torch

    tt = calibrate.solution_intervals(torch.from_numpy(t), 8)
    assert torch.is_tensor(tt) and tt.dtype == torch.int32 and tt.tolist() == out.tolist()
    with pytest.raises(ValueError, match="dumps_per_interval"):
        calibrate.solution_intervals(t, 0)
    with pytest.raises(ValueError, match="time_index"):
        calibrate.solution_intervals(np.array([-1, 0]), 2)


@pytest.mark.parametrize("n_ant, n_rows", [(5, 30), (7, 50), (12, 66 * 16)])
def test_baseline_indices_follow_uvw_tracks(n_ant, n_rows):
    a1, a2, t = synthetic.baseline_indices(n_rows, n_ant)
    nbl = n_ant * (n_ant - 1) // 2
    assert a1.dtype == a2.dtype == t.dtype == np.int32 and len(a1) == len(a2) == len(t) == n_rows
    assert np.all(a1 < a2) and a2.max() == n_ant - 1 and np.array_equal(t, np.arange(n_rows) // nbl)
    p, q = np.triu_indices(n_ant, 1)
    assert np.array_equal(a1[:nbl], p[: min(nbl, n_rows)]) and np.array_equal(a2[:nbl], q[: min(nbl, n_rows)])
    # the baseline of row r is enu[a2] - enu[a1], rotated: repeat uvw_tracks' rotation on the indexed baselines
    kw = dict(array_radius_m=900.0, dump_s=120.0, seed=5)
    uvw = synthetic.uvw_tracks(n_rows, n_ant, **kw)
    enu = synthetic.antenna_positions(n_ant, 900.0, np.random.default_rng(5))
    bl = enu[a2] - enu[a1]
    lat, dec = np.radians(-30.7), np.radians(-30.0)
    x = -np.sin(lat) * bl[:, 1] + np.cos(lat) * bl[:, 2]
    y = bl[:, 0]
    z = np.cos(lat) * bl[:, 1] + np.sin(lat) * bl[:, 2]
    n_times = -(-n_rows // nbl)
    ha = (t - (n_times - 1) / 2.0) * 120.0 * 7.292115e-5
    u = np.sin(ha) * x + np.cos(ha) * y
    v = -np.sin(dec) * np.cos(ha) * x + np.sin(dec) * np.sin(ha) * y + np.cos(dec) * z
    w = np.cos(dec) * np.cos(ha) * x - np.cos(dec) * np.sin(ha) * y + np.sin(dec) * z
    assert np.allclose(np.stack([u, v, w], axis=1), uvw, rtol=0.0, atol=1e-9)


def test_random_gains():
    g = synthetic.random_gains(3, 7, 0.2, 0.6, np.random.default_rng(1))
    assert g.shape == (3, 7) and g.dtype == np.complex128
    assert np.all(np.abs(np.abs(g) - 1.0) <= 0.2 + 1e-12) and np.all(np.abs(np.angle(g)) <= 0.6 + 1e-12)
    assert np.array_equal(g, synthetic.random_gains(3, 7, 0.2, 0.6, np.random.default_rng(1)))
    unit = synthetic.random_gains(2, 4, 0.0, 0.5, np.random.default_rng(2))
    assert np.allclose(np.abs(unit), 1.0, rtol=0.0, atol=1e-15)


# ---- the numpy statement on noise-free data -------------------------------------------
def noise_free_case(n_ant=8, n_dumps=6, nchan=4, n_int=2, seed=11, vis_dtype=np.complex64, wgt_dtype=np.float32,
                    amp=0.2, phase=0.6):
    """Noise-free corrupted data: (vis, model, wgt, ant1, ant2, interval, true gains)."""
    rng = np.random.default_rng(seed)
    nbl = n_ant * (n_ant - 1) // 2
    a1, a2, t = synthetic.baseline_indices(nbl * n_dumps, n_ant)
    interval = calibrate.solution_intervals(t, -(-n_dumps // n_int))
    model = (rng.standard_normal((len(a1), nchan)) + 1j * rng.standard_normal((len(a1), nchan))).astype(vis_dtype)
    gains = synthetic.random_gains(n_int, n_ant, amp, phase, rng)
    vis = (gains[interval, a1][:, None] * model.astype(np.complex128)
           * np.conj(gains[interval, a2])[:, None]).astype(vis_dtype)
    wgt = rng.uniform(0.5, 1.5, size=vis.shape).astype(wgt_dtype)
    wgt[rng.random(vis.shape) < 0.05] = 0.0
    return vis, model, wgt, a1, a2, interval, gains


@pytest.mark.parametrize("phase_only, bound", [(False, 40), (True, 40)])
def test_numpy_statement_recovers_noise_free_gains(phase_only, bound):
    vis, model, wgt, a1, a2, interval, truth = noise_free_case(amp=0.0 if phase_only else 0.2)
    got, ant_ok, iters, info, scale, counts = _cal_np.gaincal(vis, model, wgt, a1, a2, interval, 8, 2, niter=100,
                                                              tol=1e-10, refant=0, phase_only=phase_only)
    assert ant_ok.all() and info["n_converged"] == 2 and info["n_dead"] == 0 and info["ref_missing"] == 0
    assert iters.max() <= bound and info["max_iter_done"] == iters.max()
    # complex64 data: the model carries the rounding of vis (6e-8 relative), the solve averages it down
    err = np.abs(got - _cal_np.rotate_to(truth, 0)).max()
    print(f"phase_only={phase_only}: iterations {iters.tolist()}, gain error {err:.3g}")
    assert err <= 1e-6
    assert counts["n_added"] + counts["n_zero"] == vis.size and counts["n_zero"] == int((wgt == 0).sum())
    assert np.all(got[:, 0].imag == 0.0) or np.abs(got[:, 0].imag).max() < 1e-16  # rotated to antenna 0


def test_fixed_point_sums_are_close_to_fp64_and_order_free():
    vis, model, wgt, a1, a2, interval, _ = noise_free_case(vis_dtype=np.complex128, wgt_dtype=np.float64)
    amax, wmax = _cal_np.sample_max(vis, model, wgt, a1, a2, interval, 8, 2)
    scale = _cal_np.scale_init(8, 2, amax, wmax, vis.size)
    corr, _ = _cal_np.correlate(vis, model, wgt, a1, a2, interval, scale)
    exact = np.zeros(corr.shape)
    c = wgt * vis * np.conj(model)
    np.add.at(exact, (interval, a1, a2, 0), c.real.sum(axis=1))
    np.add.at(exact, (interval, a1, a2, 1), c.imag.sum(axis=1))
    np.add.at(exact, (interval, a1, a2, 2), (wgt * np.abs(model) ** 2).sum(axis=1))
    assert np.abs(corr * scale["quantum"] - exact).max() <= 1e-13 * np.abs(exact).max()
    assert np.abs(corr).max() < 2 ** 62
    # any split and any row order: the same integers
    perm = np.random.default_rng(0).permutation(len(a1))
    half = len(a1) // 2
    parts = None
    for sel in (perm[:half], perm[half:]):
        parts, _ = _cal_np.correlate(vis[sel], model[sel], wgt[sel], a1[sel], a2[sel], interval[sel], scale, parts)
    assert np.array_equal(parts, corr)
    # a folded row (ant1 > ant2, conjugated data) adds what the row itself adds
    swapped, _ = _cal_np.correlate(np.conj(vis), np.conj(model), wgt, a2, a1, interval, scale)
    assert np.array_equal(swapped, corr)


def test_numpy_apply_round_trip_and_dead_antenna():
    vis, _, wgt, a1, a2, interval, gains = noise_free_case(vis_dtype=np.complex128, wgt_dtype=np.float64)
    ok = np.ones(gains.shape, dtype=np.uint8)
    ok[1, 3] = 0
    bad, wbad = _cal_np.apply(vis, wgt, a1, a2, interval, gains, ok, "corrupt")
    dead_rows = (interval == 1) & ((a1 == 3) | (a2 == 3))
    assert dead_rows.any() and np.array_equal(bad[dead_rows], vis[dead_rows]) and np.all(wbad[dead_rows] == 0.0)
    assert np.array_equal(wbad[~dead_rows], wgt[~dead_rows])
    back, wback = _cal_np.apply(bad, wbad, a1, a2, interval, gains, ok, "correct")
    assert np.allclose(back, vis, rtol=1e-14, atol=0.0)
    h2 = np.abs(gains[interval, a1] * np.conj(gains[interval, a2])) ** 2
    assert np.allclose(wback[~dead_rows], (wgt * h2[:, None])[~dead_rows], rtol=1e-14)


def test_python_entry_points(monkeypatch):
    import inspect

    import torch

    import ska_sdp_cip_amd as pkg
    from ska_sdp_cip_amd import _call

    assert pkg.calibrate is calibrate and "calibrate" in pkg.__all__
    for name in ("solution_intervals", "GainCorrelator", "device_gain_correlate", "device_gain_solve",
                 "device_gain_apply", "device_gaincal", "device_selfcal", "gaincal", "gain_apply"):
        assert getattr(pkg, name) is getattr(calibrate, name) and name in pkg.__all__, name
    for name in ("baseline_indices", "random_gains"):
        assert callable(getattr(synthetic, name))
    params = inspect.signature(calibrate.device_selfcal).parameters
    assert list(params)[:9] == ["uvw", "freq", "vis", "wgt", "ant1", "ant2", "interval", "npix", "pixsize"]
    assert params["phase_only"].default is True and params["refant"].default == 0
    assert params["solver_niter"].default == 50 and params["solver_tol"].default == 1e-8
    assert params["n_rounds"].kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(calibrate.device_gain_apply).parameters["mode"].default == "correct"
    for method in ("add_ms", "all_reduce", "solve"):
        assert callable(getattr(calibrate.GainCorrelator, method))
    # the existing synthetic signatures stay as they are
    assert list(inspect.signature(synthetic.make_measurement_set).parameters)[:2] == ["n_rows", "nchan"]
    monkeypatch.setattr(_call.torch.cuda, "is_available", lambda: False)
    v = np.zeros((3, 2), dtype=np.complex64)
    cols = [np.zeros(3, dtype=np.int32)] * 3
    with pytest.raises(RuntimeError, match="needs a ROCm GPU"):
        calibrate.gaincal(v, v, np.ones((3, 2), dtype=np.float32), *cols, 2, 1)
    with pytest.raises(RuntimeError, match="needs a ROCm GPU"):
        calibrate.gain_apply(v, None, *cols, np.ones((1, 2), dtype=np.complex128))
    with pytest.raises(RuntimeError, match="needs a ROCm GPU"):
        calibrate.device_gain_apply(torch.zeros((3, 2), dtype=torch.complex64), None, *[torch.zeros(3)] * 3,
                                    torch.ones((1, 2), dtype=torch.complex128), torch.ones((1, 2)))
