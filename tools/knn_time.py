"""Timing driver for gnss_knn_classify at the size of a config-5 record set against a training set
of ten such sets: Q = 29 088 query rows, M = 290 880 training rows, D = 11 columns, k = 15, three
classes (seeded: three overlapping clusters, so the neighbours' classes are mixed). The model is
resident (GNSS_KNN_MODEL_DEVICE: uploaded once, as a caller that classifies many record sets keeps
it). In one process, after a warm-up of each:
  ROUNDS alternating rounds of (a) the device call and (b) the host path (up to 16 threads), each
  under a host clock (the device call ends in a synchronise of the context's stream, so the
  queries' upload, both kernels and the outputs' download are inside); the medians; the two
  results compared bit for bit.
With --trace the process makes the warm-up device call and two more and nothing else: run it under
`rocprofv3 --kernel-trace --stats -- python tools/knn_time.py --trace` for the kernels' durations.
The operations the definition needs are counted here from the shapes.
Args: [--trace] [ROUNDS] [OUTFILE]."""
import ctypes as C
import importlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (PyTorch's runtime first)

pkg = importlib.import_module("assignment-for-aae6102_gnss-sdr_amd")
import srcdigest  # noqa: E402

args = [a for a in sys.argv[1:] if a != "--trace"]
TRACE = "--trace" in sys.argv[1:]
ROUNDS = int(args[0]) if args else 3
OUT = args[1] if len(args) > 1 else None
Q, M, D, K, NC = 29088, 290880, 11, 15, 3
abi = pkg.abi
ctx = pkg.Context(0)
lib = ctx.lib

rng = np.random.default_rng(20240611)
y = rng.integers(0, NC, size=M).astype(np.int32)
X = rng.normal(0.0, 1.0, size=(M, D)) + 0.8 * y[:, None]
Xq = rng.normal(0.0, 1.0, size=(Q, D)) + 0.8 * rng.integers(0, NC, size=Q)[:, None]
model = pkg.knn_train(X, y, n_class=NC, ctx=ctx)


class Out:
    def __init__(self):
        self.label = np.zeros(Q, dtype=np.int32)
        self.votes = np.zeros((Q, NC), dtype=np.int32)
        self.nn_index = np.zeros((Q, K), dtype=np.int32)
        self.nn_d2 = np.zeros((Q, K))
        o = abi.GnssKnnOut()
        o.label, o.votes = self.label.ctypes.data, self.votes.ctypes.data
        o.nn_index, o.nn_d2 = self.nn_index.ctypes.data, self.nn_d2.ctypes.data
        self.c = o


cfg = abi.GnssKnnCfg()
cfg.k = K


def call(h, cm, out):
    t = time.perf_counter()
    st = lib.gnss_knn_classify(h, C.byref(cfg), C.byref(cm), Xq.ctypes.data, Q, C.byref(out.c))
    dt = time.perf_counter() - t
    if st != abi.OK:
        raise abi.GnssError(st, (lib.gnss_last_error(h) or b"").decode() if h else "")
    return dt * 1e3


d_model, h_model = model.c_model(True), model.c_model(False)
d_out, h_out = Out(), Out()
call(ctx.h, d_model, d_out)  # warm-up: the code objects and the context's scratch
if TRACE:
    call(ctx.h, d_model, d_out), call(ctx.h, d_model, d_out)
    model.free()
    ctx.close()
    sys.exit(0)

call(None, h_model, h_out)
t_dev, t_host = [], []
for _ in range(ROUNDS):
    t_dev.append(call(ctx.h, d_model, d_out))
    t_host.append(call(None, h_model, h_out))
same = all(getattr(d_out, f).tobytes() == getattr(h_out, f).tobytes() for f in ("label", "votes", "nn_index", "nn_d2"))

# what the definition needs, from the shapes: per (query, training row) D subtracts, D multiplies
# and D - 1 adds, each rounded on its own (the compare of the admission test, the insertions and
# the vote not counted); per query D subtract-multiply pairs of its standardisation
flop = Q * M * (3 * D - 1) + Q * 2 * D
# the device plan, as csrc/knn.h's knn_split_share makes it
CUS = torch.cuda.get_device_properties(0).multi_processor_count
LDS = K * 256 * 12 + 64 * D * 8  # the scan's block: the lanes' k-lists and the tile
_want = max(1, min(64, CUS * min(8, 160 * 1024 // LDS) // -(-Q // 256)))
SHARE = max(1024, -(-(-(-M // _want)) // 64) * 64)
SPLITS = -(-M // SHARE)
med = statistics.median
lines = [f"src_digest {srcdigest.src_digest()} commit {srcdigest.head_commit()}",
         f"Q {Q} queries x M {M} training rows x D {D}, k {K}, {NC} classes, resident model, seeded; {ROUNDS} "
         f"alternating rounds after one warm-up of each",
         f"per (query, row) {3 * D - 1} fp64 operations: {flop / 1e9:.1f} GFLOP in all; the standardised rows "
         f"{M * D * 8 / 1e6:.1f} MB; {SPLITS} splits of {SHARE} rows, their lists {SPLITS * K * Q * 12 / 1e6:.1f} MB",
         f"(a) device call (host clock, ends in a stream synchronise), ms: median {med(t_dev):.3f} min "
         f"{min(t_dev):.3f} max {max(t_dev):.3f}",
         f"(b) host path, up to 16 threads, ms: median {med(t_host):.1f} min {min(t_host):.1f} max {max(t_host):.1f}",
         f"labels: {np.bincount(d_out.label + 1, minlength=NC + 1).tolist()} (none, then per class); "
         f"unanimous votes {int((d_out.votes.max(axis=1) == K).sum())}",
         f"device outputs == host outputs bit for bit: {same}"]
text = "\n".join(lines) + "\n"
print(text)
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as fh:
        fh.write(text)
model.free()
ctx.close()
sys.exit(0 if same else 1)
