"""extract_DF_F_endoscope on one rank of an nccl (= RCCL) group with force_collectives: the projection goes through df_fetch, the all-reduce and df_load, and
must give the bits of the unsharded run (the sum over one rank is the rank's own).  The recording of tests/df_cases.py.  Run on a GPU box:
python scripts/df_nccl_smoke.py"""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle")); sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29537")
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
import torch, torch.distributed as td
torch.cuda.set_device(0)
td.init_process_group(backend="nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
import df_cases
from cnmf_e_amd.engine import Engine
from cnmf_e_amd.sources2d import PatchedVideo, Sources2D, Options
f, Y = df_cases.recording()
def build():
    eng = Engine(0)
    v = PatchedVideo(df_cases.D1, df_cases.D2, df_cases.T, df_cases.PATCH, 5, eng)
    v.upload_from_full(Y)
    return Sources2D(v, Options(ring_radius=5, maxIter=3, df_prctile=20, df_window=50), f.A_init, f.C_init, f.sn, dist_group=td.group.WORLD)
ref, frc = build(), build()
for s in (ref, frc):
    s.update_background_parallel(); s.update_spatial_parallel(); s.update_temporal_parallel()
frc.force_collectives = True
a, b = ref.extract_DF_F_endoscope(want_Yf=True), frc.extract_DF_F_endoscope(want_Yf=True)
assert all(np.array_equal(x, y) for x, y in zip(a, b)), [float(np.abs(x - y).max()) for x, y in zip(a, b)]
print("dF/F forced collectives: equal bits")
td.destroy_process_group()
