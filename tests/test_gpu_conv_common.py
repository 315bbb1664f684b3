"""GPU: the contract that csrc/bgnn_conv_common.h owns for the three step-2 convs -- GraphSAGE, GCN and GAT draw the SAME feature
dropout mask for the same (seed, row, column, row width) -- and the backward row pass they share without an epilogue.

One 300-row graph (a by-destination CSR with one self loop per row, about 3 000 random edges) serves all three; 300 rows cross a
block's row tile at every rung of the width ladder.  Tables are strictly positive and the bias / root is about 10, so that the
pre-activation is positive everywhere and "kept" is the same as y > 0 (ReLU and ELU are the identity there)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, E, SEED, P_DROP = 300, 3000, 4321, 0.5
DS = (1, 2, 5, 31, 64, 128)
GRAD_BAR = 2e-5          # tests/test_gpu_graphsage.py: gradients within 2e-5 of the tensor's max (+ 1e-6)


def _dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def graph():
    from bridged_gnn_amd.gcn import GcnGraph
    rng = np.random.default_rng(17)
    ei = rng.integers(0, N, size=(2, E)).astype(np.int64)
    g = GcnGraph(torch.from_numpy(ei).to(_dev()), N)
    deg = (g.csr.rowptr[1:] - g.csr.rowptr[:-1]).cpu()
    assert int(deg.min()) >= 1 and E <= g.csr.num_edges <= E + N
    return g


def _inputs(D):
    from bridged_gnn_amd import ops
    gen = torch.Generator().manual_seed(100 + D)
    Dp = ops.pad4(D)
    tbl = (0.1 + torch.rand(N, Dp, generator=gen)).to(_dev())
    bias = (10.0 + torch.rand(Dp, generator=gen)).to(_dev())
    return tbl, bias


def _sage(g, D, seed, seed_dev=None):
    from bridged_gnn_amd import ops
    tbl, bias = _inputs(D)
    root = bias.unsqueeze(0).expand(N, -1).contiguous()
    y = ops.sage_mean_aggregate(tbl, g.csr.rowptr, g.col, N, D, root=root, epilogue="relu", p_drop=P_DROP, seed=seed, seed_dev=seed_dev)
    return (y[:, :D] > 0).cpu()


def _gcn(g, D, seed, seed_dev=None):
    from bridged_gnn_amd import ops
    tbl, bias = _inputs(D)
    y = ops.gcn_aggregate(tbl, g.csr.rowptr, g.col, g.dinv, N, D, bias=bias, epilogue="relu", p_drop=P_DROP, seed=seed, seed_dev=seed_dev)
    return (y[:, :D] > 0).cpu()


def _gat(g, D, seed):
    from bridged_gnn_amd import ops
    tbl, bias = _inputs(D)
    gen = torch.Generator().manual_seed(7)
    att = torch.randn(2, D, generator=gen).to(_dev())
    s_src, s_dst = ops.gat_scores(tbl, att[0], att[1], 1, D)
    y = ops.gat_aggregate(tbl, s_src, s_dst, g.csr.rowptr, g.col, N, 1, D, bias=bias, p_att=0.0, epilogue="elu", p_drop=P_DROP, seed=seed)[0]
    return (y[:, :D] > 0).cpu()


def _non_vacuous(keep, what):
    """Between 40 % and 60 % kept from 300 elements on: at 300 fair draws 40 % lies about 3.5 standard deviations from half."""
    frac = float(keep.float().mean())
    print(f"{what}: kept {frac:.4f} of {keep.numel()}")
    if keep.numel() >= 300 and keep.shape[1] > 1:
        assert 0.4 <= frac <= 0.6, f"{what}: kept {frac:.4f}"
    else:
        assert 0.0 < frac < 1.0, f"{what}: the pattern is {'all kept' if frac else 'all dropped'}"


@pytest.mark.parametrize("D", DS)
def test_three_convs_draw_the_same_mask(graph, D):
    sage, gcn, gat = _sage(graph, D, SEED), _gcn(graph, D, SEED), _gat(graph, D, SEED)
    for keep, what in ((sage, "sage"), (gcn, "gcn"), (gat, "gat")):
        _non_vacuous(keep, f"D={D} {what}")
    assert torch.equal(sage, gcn), f"D={D}: GraphSAGE and GCN masks differ in {int((sage != gcn).sum())} elements"
    assert torch.equal(sage, gat), f"D={D}: GraphSAGE and GAT masks differ in {int((sage != gat).sum())} elements"


def test_second_column_slice_draws_the_same_mask(graph):
    D = 132                                          # a second launch at column offset c0 = 128
    sage, gcn = _sage(graph, D, SEED), _gcn(graph, D, SEED)
    _non_vacuous(sage, "D=132 sage")
    _non_vacuous(sage[:, 128:], "D=132 sage, second slice")
    assert torch.equal(sage, gcn), f"D=132: GraphSAGE and GCN masks differ in {int((sage != gcn).sum())} elements"


@pytest.mark.parametrize("D", DS + (132,))
def test_seed_plus_device_word_is_the_seed(graph, D):
    k = 1000
    word = torch.tensor([k], dtype=torch.int64, device=_dev())
    for conv, what in ((_sage, "sage"), (_gcn, "gcn")):
        want = conv(graph, D, SEED + k)
        _non_vacuous(want, f"D={D} {what}")
        assert torch.equal(conv(graph, D, SEED, seed_dev=word), want), f"D={D} {what}: seed + device word is not the seed"


def test_sage_backward_without_epilogue_needs_no_y(graph):
    """The row pass must not touch `y` when no epilogue reads it: grad_root is grad_y, grad_tbl its mean-transpose."""
    from bridged_gnn_amd import ops
    g, dev = graph, _dev()
    rowptr, col = g.csr.rowptr.cpu().long(), g.col.cpu().long()
    deg = (rowptr[1:] - rowptr[:-1])
    dst = torch.repeat_interleave(torch.arange(N), deg)
    for D in (5, 64, 132):
        Dp = ops.pad4(D)
        gen = torch.Generator().manual_seed(200 + D)
        dy = torch.randn(N, Dp, generator=gen)
        dy[:, D:] = 0
        gt, gr = ops.sage_mean_aggregate_bwd(None, dy.to(dev), g.csr.rowptr, g.t_rowptr, g.t_dst, N, D, epilogue=None)
        assert torch.equal(gr[:, :D].cpu(), dy[:, :D]), f"D={D}: grad_root is not grad_y"
        ref = torch.zeros(N, D, dtype=torch.float64).index_add_(0, col, dy[:, :D].double()[dst] / deg.double()[dst].unsqueeze(1))
        err = float((gt[:, :D].cpu().double() - ref).abs().max())
        tol = GRAD_BAR * float(ref.abs().max()) + 1e-6
        print(f"D={D}: grad_tbl max err {err:.3e} (bar {tol:.3e})")
        assert err <= tol, f"D={D}: grad_tbl max err {err:.3e} > {tol:.3e}"
