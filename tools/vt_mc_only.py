"""25-tap vector-tracking driver for timing (trackingVT_POS_updated_multicorrelator through
gnss_tracking_vt_mc) beside the plain loop's one-launch-per-step path (trackingVT_POS_updated
through gnss_tracking_vt with GNSS_OPT_NO_PERSIST = 1) in one process: the reference's 5
channels and EKF start (tests/vt_nav_common.py) on a device-resident synthetic Opensky record,
NSTEPS 1-ms steps. Per blocks-per-channel value: one warm-up call of each loop, then ITERS
timed calls alternating between them (profiling off), the median wall time per step of each and
their ratio; then one call of each with profiling on for the kernels' share (hipEvents around
each step's launches). Args: [NSTEPS] [ITERS] [NB,NB,...] [OUTFILE]."""
import importlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import torch  # noqa: F401,E402  (PyTorch's runtime first)

pkg = importlib.import_module("assignment-for-aae6102_gnss-sdr_amd")
import srcdigest  # noqa: E402
import vt_nav_common as V  # noqa: E402
from test_gpu_vt_mc import _vt_inputs  # noqa: E402

NSTEPS = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
ITERS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
NBS = [int(x) for x in sys.argv[3].split(",")] if len(sys.argv) > 3 else [15, 29, 58]
OUT = sys.argv[4] if len(sys.argv) > 4 else None
ctx = pkg.Context(0)
file, signal, acq, track, solu, cmn = pkg.initParameters()
skip = 5
cfg = pkg.synth.opensky(skip_ms=skip)
dev = pkg.DeviceRecord(ctx, (skip + NSTEPS + 60) * 58000 * 2)
pkg.synth.generate_device(ctx, cfg, dev)
file.skip, file.dev, file.data = skip, dev, None
z = V.fixture()
Acquired, eph, sbf, ct, ct_long, ns = _vt_inputs(pkg, z, skip)
xyz = V.cnslxyz(pkg)
lines = [f"src_digest {srcdigest.src_digest()} commit {srcdigest.head_commit()}",
         f"{NSTEPS} steps x {len(Acquired.sv)} channels, int8 I/Q device-resident record; us per step = wall / steps, "
         f"median of {ITERS} calls after one warm-up call each, the two loops alternating; kernel = hipEvents around "
         "each step's launch in a separate call with profiling on"]


def run(mc):
    t = time.perf_counter()
    if mc:
        _, nsol = pkg.trackingVT_POS_updated_multicorrelator(file, signal, track, cmn, solu, Acquired, xyz, eph, sbf,
                                                             None, ct_long, ns, ctx=ctx, nsteps=NSTEPS)
    else:
        _, nsol = pkg.trackingVT_POS_updated(file, signal, track, cmn, solu, Acquired, xyz, eph, sbf, None, ct, ns,
                                             ctx=ctx, nsteps=NSTEPS)
    wall = time.perf_counter() - t
    tm = ctx.timing()
    assert tm["track_launches"] == NSTEPS
    return wall / NSTEPS * 1e6, tm["track_kernel_ms"] / NSTEPS * 1e3


ctx.set_option(pkg.abi.OPT_NO_PERSIST, 1)  # the plain loop's one-launch-per-step path (vt_step_kernel)
for nb in NBS:
    ctx.set_option(pkg.abi.OPT_VT_BLOCKS, nb)
    ctx.set_profiling(False)
    run(True), run(False)
    w = {True: [], False: []}
    for it in range(ITERS):
        for mc in (True, False):
            w[mc].append(run(mc)[0])
    ctx.set_profiling(True)
    k_mc, k_pl = run(True)[1], run(False)[1]
    m_mc, m_pl = statistics.median(w[True]), statistics.median(w[False])
    lines.append(f"nb {nb:4d}: 25-tap {m_mc:7.1f} us/step (min {min(w[True]):.1f}, max {max(w[True]):.1f}; kernel "
                 f"{k_mc:.1f}), plain one-launch {m_pl:7.1f} us/step (min {min(w[False]):.1f}, max {max(w[False]):.1f}; "
                 f"kernel {k_pl:.1f}), ratio {m_mc / m_pl:.2f}")
    print(lines[-1], flush=True)
text = "\n".join(lines) + "\n"
print(text)
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as fh:
        fh.write(text)
