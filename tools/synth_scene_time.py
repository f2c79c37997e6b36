"""Timing driver for the synthetic-IF generators: 1 s (58 000 000 samples, 116 MB) of the
8-satellite Opensky scene into one device record, three ways,
  A. gnss_synth_if_device (csrc/synth.hip),
  B. gnss_synth_scene_device without rays (csrc/synth_scene.hip; the same bytes as A),
  C. gnss_synth_scene_device with two rays per satellite (16 rays, all present),
in one process: one warm-up call of each, then ROUNDS rounds of A, B, C in turn, a host clock
around each call (every call ends in a synchronise of the context's stream, so the uploads of the
parameters, the launch and the kernel are inside). Per way the median, minimum and maximum, and as
the run-to-run spread the largest (max - min) of the three. B's bytes are compared with A's.
With --trace the process makes the warm-up calls and two more of each and nothing else: run it
under `rocprofv3 --kernel-trace --stats -- python tools/synth_scene_time.py --trace` for the
kernels' own durations. Args: [--trace] [ROUNDS] [OUTFILE]."""
import importlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import torch  # noqa: E402,F401  (PyTorch's runtime first)

pkg = importlib.import_module("assignment-for-aae6102_gnss-sdr_amd")
import srcdigest  # noqa: E402

args = [a for a in sys.argv[1:] if a != "--trace"]
TRACE = "--trace" in sys.argv[1:]
ROUNDS = int(args[0]) if args else 9
OUT = args[1] if len(args) > 1 else None
N = 1000 * 58000
S = pkg.synth

ctx = pkg.Context(0)
cfg = S.opensky(skip_ms=2)
for i in range(cfg.n_sv):
    cfg.sv[i].lnav = 1
bare = S.scene_of(cfg)
rays = S.scene_of(cfg)
for k, prn in enumerate(S.OPENSKY_SV):
    S.add_ray(rays, prn, 0.3 + 0.1 * k, 0.5, phase_cycles=0.125 * k, fade_hz=1.0 + k)
    S.add_ray(rays, prn, 1.2 + 0.05 * k, 0.3, phase_cycles=0.5)
rec_a, rec_b = pkg.DeviceRecord(ctx, 2 * N), pkg.DeviceRecord(ctx, 2 * N)
WAYS = [("A gnss_synth_if_device", lambda: S.generate_device(ctx, cfg, rec_a)),
        ("B scene kernel, no rays", lambda: S.generate_scene_device(ctx, bare, rec_b)),
        ("C scene kernel, 16 rays", lambda: S.generate_scene_device(ctx, rays, rec_b))]


def timed(f):
    t = time.perf_counter()
    f()
    return (time.perf_counter() - t) * 1e3


for _, f in WAYS:
    f()  # warm-up: code objects, the context's buffers
if TRACE:
    for _ in range(2):
        for _, f in WAYS:
            f()
    ctx.close()
    sys.exit(0)

ms = {name: [] for name, _ in WAYS}
for _ in range(ROUNDS):
    for name, f in WAYS:
        ms[name].append(timed(f))
WAYS[1][1]()
same = bool((rec_a.download() == rec_b.download()).all())

med = statistics.median
spread = max(max(v) - min(v) for v in ms.values())
a, b = med(ms[WAYS[0][0]]), med(ms[WAYS[1][0]])
lines = [f"src_digest {srcdigest.src_digest()} commit {srcdigest.head_commit()}",
         f"{N} samples ({2 * N / 1e6:.0f} MB) of the 8-satellite Opensky scene (LNAV bits), {ROUNDS} rounds of A, B, C "
         "in turn after one warm-up call of each; host clock around each call, which ends in a stream synchronise"]
for name, _ in WAYS:
    v = ms[name]
    lines.append(f"{name:26s} ms: median {med(v):8.3f}  min {min(v):8.3f}  max {max(v):8.3f}   "
                 f"{N / med(v) / 1e6:7.2f} Gsample/s")
lines += [f"run-to-run spread (largest max - min of the three), ms: {spread:.3f}",
          f"B's bytes == A's bytes: {same}",
          f"condition B <= A + spread: {b <= a + spread} ({b:.3f} against {a:.3f} + {spread:.3f})"]
text = "\n".join(lines) + "\n"
print(text)
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as fh:
        fh.write(text)
rec_a.free()
rec_b.free()
ctx.close()
sys.exit(0 if same else 1)
