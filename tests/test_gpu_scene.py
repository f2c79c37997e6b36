"""GPU tests of the multipath / NLOS scene generator (gnss_synth_scene_device,
csrc/synth_scene.hip): the kernel's bytes equal the host path's on the scene and ranges of
test_scene_kat.py, at every code-table size and destination alignment; a ray-less scene equals
gnss_synth_if_device over 17 000 123 samples; the tail of that run with rays equals the host path;
chunking; the refusals, each leaving the context usable; a multi-device context's resident copies
are dropped; and, end to end, the 25-tap loop and the ACF features see the code-phase bias that
theory predicts for a half-chip ray, in phase and opposed."""
import ctypes as C

import numpy as np
import pytest

import scene_twin as T
from conftest import acquired_of, params
from test_scene_kat import bad_scenes

pytestmark = pytest.mark.gpu

LONG = 17_000_123  # more than 65 536 x 256 samples: every grid-stride loop wraps


def on_device(pkg, ctx, scene, sample0, n, pad=0):
    """The samples generated into a fresh record `pad` bytes in; the record's other bytes must
    stay as they were."""
    fill = np.full(2 * n + pad + 6, 77, dtype=np.int8)
    dev = pkg.DeviceRecord.from_host(ctx, fill)
    try:
        st = ctx.lib.gnss_synth_scene_device(ctx.h, C.byref(scene), C.c_uint64(sample0), C.c_uint64(n),
                                             C.c_void_p(dev.ptr.value + pad))
        assert st == pkg.abi.OK, ctx.lib.gnss_last_error(ctx.h)
        got = dev.download()
    finally:
        dev.free()
    assert np.all(got[:pad] == 77) and np.all(got[pad + 2 * n:] == 77)
    return got[pad: pad + 2 * n]


@pytest.fixture(scope="module")
def kat(pkg):
    return T.kat_scene(pkg)


@pytest.mark.parametrize("sample0,n", T.KAT_RANGES)
def test_device_equals_host(pkg, ctx, kat, sample0, n):
    want = pkg.synth.generate_scene_host(kat, sample0, n)
    assert T.mismatch_report(on_device(pkg, ctx, kat, sample0, n), want, sample0=sample0) == ""


@pytest.mark.parametrize("n,pad", [(1, 0), (1, 2), (2, 2), (3, 0), (777, 2), (1026, 6), (5001, 0)])
def test_device_equals_host_at_every_alignment(pkg, ctx, kat, n, pad):
    """A destination 2 bytes off a 4-byte boundary and odd counts: the single samples before and
    after the pairs. The ray edges of the first range lie inside the longer ones."""
    a = 1001 - 300
    want = pkg.synth.generate_scene_host(kat, a, n)
    assert T.mismatch_report(on_device(pkg, ctx, kat, a, n, pad), want, sample0=a) == ""


@pytest.mark.parametrize("n_sv", [8, 9, 17, 33, 64])
def test_device_equals_host_at_every_table_size(pkg, ctx, n_sv):
    """The kernel is built for 8, 16, 32 and 64 code rows in LDS."""
    prns = [1 + i % 51 for i in range(n_sv)]
    rng = np.random.Generator(np.random.PCG64(n_sv))
    cfg = pkg.synth.scenario(prns, [int(x) for x in rng.integers(0, 58000, n_sv)],
                             [float(x) for x in rng.uniform(-4000, 4000, n_sv)], [44.0] * n_sv, skip_ms=2)
    cfg.sv[n_sv - 1].lnav = 1
    sc = pkg.synth.scene_of(cfg)
    pkg.synth.add_ray(sc, prns[n_sv - 1], 0.4, 0.9, phase_cycles=0.3)
    pkg.synth.add_ray(sc, prns[0], 1.1, 0.9, fade_hz=-2.0)
    n = 4099
    want = pkg.synth.generate_scene_host(sc, 7, n)
    assert T.mismatch_report(on_device(pkg, ctx, sc, 7, n), want, sample0=7) == ""


@pytest.fixture(scope="module")
def long_cfg(pkg):
    cfg = pkg.synth.opensky(skip_ms=2)
    for i in range(cfg.n_sv):
        cfg.sv[i].lnav = 1
    return cfg


def test_rayless_scene_equals_legacy_generator(pkg, ctx, long_cfg):
    a, b = pkg.DeviceRecord(ctx, 2 * LONG), pkg.DeviceRecord(ctx, 2 * LONG)
    try:
        pkg.synth.generate_device(ctx, long_cfg, a)
        pkg.synth.generate_scene_device(ctx, pkg.synth.scene_of(long_cfg), b)
        x, y = a.download(), b.download()
    finally:
        a.free()
        b.free()
    assert T.mismatch_report(y, x) == ""


def test_tail_of_a_long_run_with_rays(pkg, ctx, long_cfg):
    sc = pkg.synth.scene_of(long_cfg)
    for k, prn in enumerate(pkg.synth.OPENSKY_SV):
        pkg.synth.add_ray(sc, prn, 0.3 + 0.1 * k, 0.5, phase_cycles=0.125 * k, fade_hz=1.0 + k)
        pkg.synth.add_ray(sc, prn, 1.2, 0.3, t_on_ms=290, t_off_ms=292.5)
    assert sc.n_ray == 16
    tail = 58000
    dev = pkg.DeviceRecord(ctx, 2 * LONG)
    try:
        pkg.synth.generate_scene_device(ctx, sc, dev)
        got = dev.download(2 * (LONG - tail), 2 * tail)
    finally:
        dev.free()
    want = pkg.synth.generate_scene_host(sc, LONG - tail, tail)
    assert T.mismatch_report(got, want, sample0=LONG - tail) == ""


def test_chunked_generation_on_the_device(pkg, ctx, kat):
    a, n, cut = 5_300_000_123, 9001, 4097
    whole = on_device(pkg, ctx, kat, a, n)
    dev = pkg.DeviceRecord(ctx, 2 * n)
    try:
        pkg.synth.generate_scene_device(ctx, kat, dev, a, cut)
        st = ctx.lib.gnss_synth_scene_device(ctx.h, C.byref(kat), C.c_uint64(a + cut), C.c_uint64(n - cut),
                                             C.c_void_p(dev.ptr.value + 2 * cut))
        assert st == pkg.abi.OK
        parts = dev.download()
    finally:
        dev.free()
    assert np.array_equal(whole, parts)


def test_device_refusals_leave_the_context_usable(pkg, ctx, kat):
    dev = pkg.DeviceRecord.from_host(ctx, np.full(2 * 64, 77, dtype=np.int8))
    try:
        for name, sc in bad_scenes(pkg):
            st = ctx.lib.gnss_synth_scene_device(ctx.h, C.byref(sc), 0, 64, dev.ptr)
            assert st == pkg.abi.EARG, name
            assert ctx.lib.gnss_last_error(ctx.h), name
            assert np.all(dev.download() == 77), name
            pkg.synth.generate_scene_device(ctx, kat, dev)  # a valid call on the same context
            assert np.array_equal(dev.download(), pkg.synth.generate_scene_host(kat, 0, 64)), name
            dev.upload(np.full(2 * 64, 77, dtype=np.int8))
        assert ctx.lib.gnss_synth_scene_device(ctx.h, None, 0, 64, dev.ptr) == pkg.abi.EARG
        assert ctx.lib.gnss_synth_scene_device(ctx.h, C.byref(kat), 0, 64, None) == pkg.abi.EARG
        assert ctx.lib.gnss_synth_scene_device(None, C.byref(kat), 0, 64, dev.ptr) == pkg.abi.EARG
    finally:
        dev.free()


@pytest.mark.parametrize("devices,peer", [([0, 0, 0], 1), ([0, 1], 0)])
def test_scene_write_drops_resident_copies(pkg, ctx, devices, peer):
    """A member's resident copy of a device record is stale once the scene generator has written
    into the record: it is dropped (gnss_ctx_resident_records), for a write of the whole record
    and of a part. Members on one GPU keep copies with OPT_FORCE_PEER; two GPUs do so always."""
    if max(devices) >= pkg.abi.load().gnss_device_count():
        pytest.skip("fewer than two devices")
    skip = 2
    cfg = pkg.synth.opensky(skip_ms=skip)
    sc = pkg.synth.scene_of(cfg)
    pkg.synth.add_ray(sc, 3, 0.5, 0.5)
    n_ms = skip + 100 + 19 + 60 + 12
    mctx = pkg.Context(devices=devices)
    dev = pkg.DeviceRecord(mctx, 2 * n_ms * 58000)
    try:
        mctx.set_option(pkg.abi.OPT_FORCE_PEER, peer)
        pkg.synth.generate_scene_device(mctx, sc, dev)
        file, signal, acq, track = params(pkg, skip, None)
        file.dev = dev
        track.msToProcessCT_1ms, track.msToProcessCT_10ms = 100, 60
        A = acquired_of([3, 16], [3683, 26051], [4580990.0, 4579695.0])
        for write in (lambda: pkg.synth.generate_scene_device(mctx, sc, dev),
                      lambda: pkg.synth.generate_scene_device(mctx, sc, dev, 1000, 33)):
            pkg.trackingCT(file, signal, track, A, ctx=mctx, raw=True)
            assert mctx.resident_records > 0
            write()
            assert mctx.resident_records == 0
    finally:
        mctx.set_option(pkg.abi.OPT_FORCE_PEER, 0)
        dev.free()
        mctx.close()


# ---- the physics, end to end ----------------------------------------------------------------
PHYS_MS = 2 + 1 + 600 + 4


@pytest.fixture(scope="module")
def physics(pkg, ctx):
    """PRN 3 alone at 55 dB-Hz without a ray, with a ray half a chip late at half the amplitude in
    phase, and with the same ray opposed: each through trackingCT_multiCorr and acf_features."""
    out = {}
    for name, phase in (("none", None), ("in_phase", 0.0), ("opposed", 0.5)):
        sc = pkg.synth.scene_of(pkg.synth.scenario([3], [3683], [990.0], [55.0], skip_ms=2))
        if phase is not None:
            pkg.synth.add_ray(sc, 3, 0.5, 0.5, phase_cycles=phase)
        dev = pkg.DeviceRecord(ctx, 2 * PHYS_MS * 58000)
        try:
            pkg.synth.generate_scene_device(ctx, sc, dev)
            file, signal, acq, track = params(pkg, 2, None)
            file.dev = dev
            tck, _ = pkg.trackingCT_multiCorr(file, signal, track, acquired_of([3], [3683], [4580990.0]),
                                              datalength=600, ctx=ctx)
        finally:
            dev.free()
        f = pkg.acf_features(tck, [3], [45.0], want_corr=True)
        out[name] = (sc, tck, f)
    return out


@pytest.mark.parametrize("name,predicted", [("none", 0.0), ("in_phase", -1.0 / 6.0), ("opposed", 0.2)])
def test_ray_biases_the_code_phase_as_predicted(physics, name, predicted):
    """The DLL 0.5(E-L)/(E+L) at +-0.5 chip locks where E = L on R(tau) +- 0.5 R(tau - 0.5): 1/6
    chip late for the in-phase ray, 0.2 chip early for the opposed one. F2 shows that in every
    window after the first, which is pull-in (600 rows from row 1 give (600 - 1) // 100 = 5
    windows: the second to the fifth), to one tap spacing (0.05 chip, the arg-max's resolution).
    Measured: -0.1555 ... -0.1485 in phase, +0.1925 ... +0.197 opposed, within 0.0015 of 0
    without a ray."""
    _, _, f = physics[name]
    assert f.windows[0] == 5
    F2 = f.F2[0]
    print(name, "F2", F2)
    assert len(F2[1:]) == 4 and np.all(np.abs(F2[1:] - predicted) <= 0.05), F2


@pytest.mark.parametrize("name,side", [("in_phase", 1), ("opposed", -1)])
def test_ray_skews_the_mean_tap_profile(physics, name, side):
    _, _, f = physics[name]
    profile = f.corr[0, :, 100:600].mean(axis=1)
    print(name, "peak tap", int(np.argmax(profile)))
    assert np.sign(int(np.argmax(profile)) - 12) == side, profile


def test_scene_labels_of_the_physics_records(pkg, physics):
    for name, want in (("none", 0), ("in_phase", 1), ("opposed", 1)):
        sc, tck, f = physics[name]
        lab = pkg.scene_labels(sc, tck, [3])[0]
        assert len(lab) == f.windows[0] and np.all(lab == want), (name, lab)
