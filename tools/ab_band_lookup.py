#!/usr/bin/env python3
"""Timing of the band launch with the look-up role (k_band_lookup_bf16x3) inside ranking passes; with a COPER_DBG_BL_CLOCK build
(tools/ab_build.py --only kernels_score3_bf16.hip blclk=-DCOPER_DBG_BL_CLOCK) also the phase boundaries of the role's workgroups
(wave 0 of each) inside the last launch.  tools/ab_band_lookup.py [workload] [Q]"""
import ctypes, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from coper_amd import data as cdata
from coper_amd.models import ConvE
name = sys.argv[1] if len(sys.argv) > 1 else "fb15k237_cpg"
Q = int(sys.argv[2]) if len(sys.argv) > 2 else 20480
md = cdata.model_descriptors(name)
m = ConvE(md, device="cuda:0", score_mode="bf16x3").load_parameters(cdata.synthetic_params(md, 0)).prepare()
q = cdata.synthetic_queries(md, Q, seed=0)
dq = {k: torch.as_tensor(v).cuda() for k, v in q.items()}
for _ in range(5):
    m.rank_pass(dq["e1"], dq["rel"], dq["e2"], dq["filt_indptr"], dq["filt_idx"], want_equal=False)
m.profile(True)
for k in ("tail", "score_count", "band_exact", "band_lookup", "dense", "group"): m.profile_read(k)
for _ in range(40):
    m.rank_pass(dq["e1"], dq["rel"], dq["e2"], dq["filt_indptr"], dq["filt_idx"], want_equal=False)
torch.cuda.synchronize()
for k in ("group", "dense", "tail", "score_count", "band_exact"):
    ms, n = m.profile_read(k)
    if n: print("%-12s avg %.4f ms (%d)" % (k, ms / n, n))
print("band launches that carried the look-up role: %d" % m.profile_read("band_lookup")[1])
try:
    lib = ctypes.CDLL(os.environ.get("COPER_HIP_LIB", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "coper_amd", "libcoper_hip.so")))
    out = (ctypes.c_double * 16)()
    if lib.coper_dbg_bl_clock(out) == 0:
        print("   grid: %d band workgroups + %d look-up workgroups; us from the earliest workgroup's start" % (out[12], out[13]))
        for i, nm in enumerate(["role start", "own entries done", "scan done", "end"]):
            print("   %-22s median %6.2f us   last workgroup %6.2f us" % (nm, out[i], out[4 + i]))
        print("   scan alone (scan done - own entries done): median %.2f us, longest %.2f us" % (out[14], out[15]))
        print("   first look-up workgroup starts at %.2f us, the last at %.2f us" % (out[8], out[9]))
        print("   band workgroups end at %.2f us in the median; the launch's last workgroup ends at %.2f us (%s)"
              % (out[11], out[10], "a look-up workgroup" if out[7] >= out[10] else "a band workgroup"))
except AttributeError:
    pass
