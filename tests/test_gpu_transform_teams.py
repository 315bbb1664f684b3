"""GPU: team mode of the hidden transform (transform_stream_kernel, GemmParams::team_*; `ops.transform_team_runs` is the plan).
Every case runs `ops.adaptedconv_transform` in this process, team mode on, and once more in ONE fresh child process for all
cases with BGNN_TS_TEAMS=0 (the library reads the switch once): the rows of every tile the need bits (or the tail groups) say
are written must be equal bit for bit, and the rows behind row N stay untouched.  The plan is part of the check: a case that is
about team mode must have a run, a case about its limits must have none."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import assert_close
from test_gpu_classifier_stage import DEV, GUARD, dev_head, domain_sums64, make_head, sentinel, untouched

pytestmark = pytest.mark.gpu

N_SRC, N_TAR = 40003, 50001          # case (a): boundary tile 1250 holds both domains, the last tile is partial
D = 128


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _st_graph(src_ids, tar_ids, seed):
    """2 within-domain in-edges per node + 2 source -> target bridge edges per target (from = neighbour, to = node)"""
    rng = np.random.default_rng(seed)
    ns, nt = len(src_ids), len(tar_ids)
    pick = lambda ids, k: ids[rng.integers(0, len(ids), k)]
    frm = np.concatenate([pick(src_ids, 2 * ns), pick(tar_ids, 2 * nt), pick(src_ids, 2 * nt)])
    to = np.concatenate([np.repeat(src_ids, 2), np.repeat(tar_ids, 2), np.repeat(tar_ids, 2)])
    return np.stack([frm, to]).astype(np.int64)


def _domains(case):
    """-> (domain flags [n] bool, True = source; graph or None; tail_single)"""
    cu = _n_cu()
    if case in ("a", "b72", "b100"):
        m = np.arange(N_SRC + N_TAR) < N_SRC
    elif case == "c":                                   # [T ; S]: the run comes first
        m = np.arange(N_SRC + N_TAR) >= N_TAR
    elif case == "d":                                   # domains interleaved every 64 rows
        m = (np.arange(20011) // 64) % 2 == 0
    elif case == "e":                                   # the target run gives every block 3 tiles (and some a 4th)
        m = np.arange(4099 + 32 * (3 * cu + cu // 2)) < 4099
    elif case == "f":                                   # tail groups: 4 tiles and a few per block need h_t2s only, a short group h_s2t only
        n_t2s, n_s2t = 32 * (4 * cu + 7) + 5, 1000
        n = 5003 + n_t2s + n_s2t
        g = torch.Generator().manual_seed(11)
        return (torch.rand(n, generator=g) < 0.5).numpy(), None, (n_t2s, n_s2t)
    ids = np.arange(len(m))
    return m, _st_graph(ids[m], ids[~m], seed=len(m)), (0, 0)


def _inputs(case):
    """host tensors of a case, the same in both processes"""
    din = {"b72": 72, "b100": 100}.get(case, 128)
    m, ei, tail = _domains(case)
    n = len(m)
    g = torch.Generator().manual_seed(1000 + n + din)
    m = torch.from_numpy(m)
    x = torch.randn(n, din, generator=g)
    x[m] += torch.randn(din, generator=g) * 0.5
    return x, m, make_head(g, D, din, True), ei, tail


def _run(case):
    """-> (h_t2s [n + GUARD], h_s2t [n + GUARD], needed rows of h_t2s [n] bool, of h_s2t, plan)"""
    from bridged_gnn_amd import ops
    x, m, head, ei, tail = _inputs(case)
    n = x.shape[0]
    m8 = m.to(DEV, torch.uint8)
    packed = ops.pack_transform_heads([dev_head(head)], x.shape[1])
    need = None
    rows = torch.arange(n, device=DEV)
    if ei is not None:
        csr = ops.build_dst_csr(torch.from_numpy(ei).to(DEV), n, rewrite_self_loops=True)
        need = csr.tile_need(m8)
        assert need is not None, "s -> t bridges only: some tile needs one table"
        w_s2t, w_t2s = (need[rows // 32] & 1).bool(), (need[rows // 32] & 2).bool()
    else:
        t2s_begin, s2t_begin = n - tail[0] - tail[1], n - tail[1]
        w_s2t, w_t2s = (rows < t2s_begin) | (rows >= s2t_begin), rows < s2t_begin
    plan = ops.transform_team_runs(n, torch.device(DEV), need, tail)
    out = (sentinel(n + GUARD, packed[4]), sentinel(n + GUARD, packed[4]))
    ops.adaptedconv_transform(x.to(DEV), m8, None, packed, out=[out], sums=domain_sums64(x, m).to(DEV), tail_single=tail, tile_need=need)
    torch.cuda.synchronize()
    return out[0], out[1], w_t2s, w_s2t, plan


CASES = ("a", "b72", "b100", "c", "d", "e", "f")


def _off_child(outdir):
    assert os.environ.get("BGNN_TS_TEAMS") == "0"
    for case in CASES:
        h_t2s, h_s2t, w_t2s, w_s2t, _ = _run(case)
        assert untouched(h_t2s[-GUARD:]) and untouched(h_s2t[-GUARD:])
        torch.save((h_t2s[:-GUARD][w_t2s].cpu(), h_s2t[:-GUARD][w_s2t].cpu()), os.path.join(outdir, case + ".pt"))


@pytest.fixture(scope="module")
def off_rows(tmp_path_factory):
    """needed rows of every case as the library writes them with BGNN_TS_TEAMS=0: one child process for all cases"""
    outdir = str(tmp_path_factory.mktemp("teams_off"))
    r = subprocess.run([sys.executable, "-s", os.path.abspath(__file__), "--off-child", outdir], env=dict(os.environ, BGNN_TS_TEAMS="0"),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    return lambda case: torch.load(os.path.join(outdir, case + ".pt"))


def _expected_plan(case):
    if case in ("a", "b72", "b100"):                    # tiles behind the boundary tile, to the partial last one: h_s2t only
        return [((N_SRC + 31) // 32, (N_SRC + N_TAR + 31) // 32, 0)]
    if case == "c":                                     # tiles in front of the boundary tile
        return [(0, N_TAR // 32, 0)]
    if case == "f":                                     # the h_t2s group qualifies, the h_s2t group is too short
        n_t2s = 32 * (4 * _n_cu() + 7) + 5
        return [((5003 + 31) // 32, (5003 + n_t2s) // 32, 1)]
    return []                                           # d: runs of two tiles; e: 3 tiles per block


@pytest.mark.parametrize("case", CASES)
def test_team_mode_equals_the_switched_off_library(case, off_rows):
    """(a) [S ; T], s -> t bridges; (b) the same with Din = 72 / 100; (c) [T ; S]: the block re-arms back; (d) interleaved domains and
    (e) a run of 3 tiles per block: the plan is empty and the launch is the one without team mode; (f) tail groups."""
    h_t2s, h_s2t, w_t2s, w_s2t, plan = _run(case)
    assert plan == _expected_plan(case), f"case {case}: plan {plan}"
    if plan:
        n_blocks = min((h_t2s.shape[0] - GUARD + 31) // 32, _n_cu())
        assert all((e - b) // n_blocks >= 4 for b, e, _ in plan)
    off_t2s, off_s2t = off_rows(case)
    got_t2s, got_s2t = h_t2s[:-GUARD][w_t2s], h_s2t[:-GUARD][w_s2t]
    assert int(w_t2s.sum()) > 0 and int(w_s2t.sum()) > 0
    assert torch.equal(got_t2s.view(torch.int32).cpu(), off_t2s.view(torch.int32)), f"case {case}: needed h_t2s rows differ"
    assert torch.equal(got_s2t.view(torch.int32).cpu(), off_s2t.view(torch.int32)), f"case {case}: needed h_s2t rows differ"
    assert not bool((got_t2s.view(torch.int32) == 0x7FA5C3E1).all(dim=1).any()), f"case {case}: a needed h_t2s row was not written"
    assert not bool((got_s2t.view(torch.int32) == 0x7FA5C3E1).all(dim=1).any()), f"case {case}: a needed h_s2t row was not written"
    assert untouched(h_t2s[-GUARD:]) and untouched(h_s2t[-GUARD:]), f"case {case}: rows behind row N written"


def test_eval_forward_on_the_team_graph_vs_c_oracle():
    """(g) case (a)'s graph through the model's eval forward (the hidden conv's transform runs in team mode) against the C oracle's
    full forward at the default bar"""
    from bridged_gnn_amd import ops
    from bridged_gnn_amd.data import Data
    from bridged_gnn_amd.ktgnn import KTGNN_no_complement
    from oracle import oracle_c as OC
    from oracle import oracle_np as O
    x, m, _, ei, _ = _inputs("a")
    n = x.shape[0]
    need = ops.build_dst_csr(torch.from_numpy(ei).to(DEV), n, rewrite_self_loops=True).tile_need(m.to(DEV, torch.uint8))
    assert ops.transform_team_runs(n, torch.device(DEV), need) == _expected_plan("a")
    torch.manual_seed(5)
    model = KTGNN_no_complement(128, 2, 2, 128, root_weight=False, use_bn=True, dim_share=128, need_complement=False)
    g = torch.Generator().manual_seed(3)
    for mod in model.modules():
        if isinstance(mod, torch.nn.BatchNorm1d):
            mod.running_mean.copy_(torch.randn(mod.num_features, generator=g) * 0.1)
            mod.running_var.copy_(torch.rand(mod.num_features, generator=g) + 0.5)
    model = model.to(DEV).eval()
    data = Data(x=x.to(DEV), edge_index=torch.from_numpy(ei).to(DEV), central_mask=m.to(DEV))
    with torch.no_grad():
        out = [t.cpu().numpy() for t in model(data)[:3]]
        emb = model.get_emb(data).cpu().numpy()[:, :128]
    sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    rowptr, col, _ = O.dst_csr(ei, m.numpy())
    rb, rt, rth, remb = OC.ktgnn_forward_eval(x.numpy(), rowptr, col, m.numpy(), sd, return_emb=True)
    for name, got, ref in (("hidden conv (BN+ReLU)", emb, remb), ("logp_base", out[0], rb), ("logp_target", out[1], rt), ("logp_target_hat", out[2], rth)):
        assert_close(got, ref, what=f"{name}, team graph")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--off-child":
        _off_child(sys.argv[2])
