"""world_size-2 gloo test of the SHARDED second pass on the CPU: Sources2D.initComponents_residual_parallel with the patches of case P split over two ranks must
append what the single-process oracle finds (the all-reduce of the counts, the all-gather of the new footprints, the all-reduce of the packed rows and of the
images: Sources2D._stitch_init, shared with initComponents_parallel).  Kernels are the test double of tests/test_residual_oracle.py; what is under test is the
distributed host logic."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


def _worker(rank, world, port, out):
    for p_ in (ROOT, os.path.join(ROOT, "oracle"), HERE):
        sys.path.insert(0, p_)
    import torch.distributed as td
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    td.init_process_group("gloo", rank=rank, world_size=world)
    import residual_cases as rc
    from test_residual_oracle import _double
    from cnmf_e_amd.sources2d import PatchedVideo, Sources2D
    c = rc.CASES["P"]
    f, Y, A0, C0 = rc.inputs("P")
    d1, d2 = c["dims"]
    eng = _double()
    eng.gSig, eng.gSiz = c["gSig"], c["gSiz"]
    video = PatchedVideo(d1, d2, c["T"], rc.pdims(c), c["r"], eng, rank=rank, world_size=world)
    assert len(video.owned) == 4 // world
    video.upload_from_full(Y.astype(np.float64))
    s = Sources2D(video, rc.options("P"), A0, C0, f.sn, dist_group=td.group.WORLD)
    s.update_background_parallel()
    center, Cn, PNR = s.initComponents_residual_parallel(min_corr=c["min_corr"], min_pnr=c["min_pnr"])
    np.savez(out % rank, A=s.A.toarray(), C=np.asarray(s.C), C_raw=np.asarray(s.C_raw), S=np.asarray(s.S), center=center, Cn=Cn, PNR=PNR, ids=s.ids, k_ids=s.P["k_ids"])
    td.barrier()
    td.destroy_process_group()


def test_two_rank_sharded_second_pass_matches_the_oracle(tmp_path):
    import torch.multiprocessing as mp
    sys.path.insert(0, HERE)
    import residual_cases as rc
    from test_distributed_cpu import _free_port
    out = str(tmp_path / "r%d.npz")
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    r0, r1 = np.load(out % 0), np.load(out % 1)
    for key in r0.files:                                                  # every rank holds the same result
        assert np.array_equal(r0[key], r1[key]), key
    c = rc.CASES["P"]
    ora = rc.oracle("P")
    K_old, K_new = c["K"] - c["hold"], ora["center"].shape[0]
    assert K_new >= 2 and np.array_equal(r0["center"], ora["center"])     # patches in column-major order whichever rank owns them
    assert r0["A"].shape == (c["dims"][0] * c["dims"][1], K_old + K_new) and r0["C"].shape == r0["C_raw"].shape == r0["S"].shape == (K_old + K_new, c["T"])
    got_A = r0["A"][:, K_old:].astype(np.float64)
    assert np.array_equal(got_A != 0, ora["A"].astype(np.float32) != 0) and np.allclose(got_A, ora["A"], rtol=1e-6, atol=0)
    assert np.allclose(r0["C"][K_old:], ora["C"], rtol=1e-5, atol=1e-5) and np.allclose(r0["C_raw"][K_old:], ora["C_raw"], rtol=1e-5, atol=1e-5)
    assert np.array_equal(r0["ids"], np.arange(1, K_old + K_new + 1)) and int(r0["k_ids"]) == K_old + K_new
    assert r0["Cn"].shape == tuple(c["dims"]) and np.isfinite(r0["Cn"]).all() and r0["PNR"].any()
