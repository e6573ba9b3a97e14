"""profiling helper: discretize_kernel of several builds of libmpcx.so in turn on one box -- HIP events around
mpcx_discretize_stages_ragged_dev on a benchmark workload, each build in a process of its own, several rounds
usage: python profiles/tools/discretize_ab.py [--rounds N] [--workload S4096_K30] libA.so libB.so ..."""
import os, subprocess, sys
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
CODE = '''
import sys
sys.path.insert(0, %r)
import ctypes as C
from mpconstellation_amd import _ffi
_ffi.LIB_PATH = %r
import torch, bench
r = bench.Runner(%r, 0, 1, 0)
p = lambda t: C.c_void_p(t.data_ptr()); st = C.c_void_p(r.stream)
ms = []
for rep in range(12):
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True); e0.record()
    _ffi.check(r.lib.mpcx_discretize_stages_ragged_dev(r.ctx, r.S, r.K, None, r.K, None, p(r.d_x), p(r.d_u), p(r.d_tf), p(r.d_c), 0, 1e-2, p(r.d_stage), p(r.d_dst), st), r.ctx, "discretize")
    e1.record(); torch.cuda.synchronize(); ms.append(e0.elapsed_time(e1))
ms = sorted(ms[2:])
print("%%-28s discretize_kernel min %%.4f median %%.4f max %%.4f ms (10 launches), status ok %%d/%%d" %% (%r, ms[0], ms[len(ms) // 2], ms[-1], int((r.d_dst == 0).sum()), r.S), flush=True)
'''
args = sys.argv[1:]
rounds, wl = 3, "S4096_K30"
while args and args[0].startswith("--"):
    if args[0] == "--rounds": rounds = int(args[1])
    elif args[0] == "--workload": wl = args[1]
    else: raise SystemExit(__doc__)
    args = args[2:]
for rnd in range(rounds):
    print(f"round {rnd + 1}", flush=True)
    for lib in args:
        subprocess.run([sys.executable, "-c", CODE % (ROOT, os.path.abspath(lib), wl, os.path.relpath(lib))], check=True, timeout=120)
