"""GPU: the need-mask transform (bgnn_adaptedconv_transform_f32 with tile_need_opt, `ops.adaptedconv_transform(..., tile_need=...)`) at its own
interface: a table's rows in a tile whose need bit is set are bit-equal to the unmasked call, rows of a tile whose bit is clear
are either untouched or exactly the unmasked value, guard rows stay untouched, and the unmasked call meets the default bar
against fp64 (the restatement of tests/test_gpu_classifier_stage.py, itself checked against the C oracle there)."""
import pytest
import torch

from test_gpu_classifier_stage import DEV, GUARD, SENTINEL, close, dev_head, domain_sums64, make_head, ref_transform, sentinel, untouched

pytestmark = pytest.mark.gpu

NEEDS = ("all3", "all1", "all2", "all0", "mix")


def _setup(din, D, n, seed):
    from bridged_gnn_amd import ops
    g = torch.Generator().manual_seed(seed)
    m = torch.rand(n, generator=g) < 0.45
    m[0], m[n - 1] = True, False
    x = torch.randn(n, din, generator=g)
    x[m] += torch.randn(din, generator=g) * 0.5
    head = make_head(g, D, din, True)
    sums = domain_sums64(x, m)
    packed = ops.pack_transform_heads([dev_head(head)], din)
    return x, m, head, sums, packed, g


def _run(x, m, sums, packed, need):
    """-> (h_t2s, h_s2t) sentinel-filled tables of n + GUARD rows after one call"""
    from bridged_gnn_amd import ops
    n, ldh = x.shape[0], packed[4]
    out = (sentinel(n + GUARD, ldh), sentinel(n + GUARD, ldh))
    ops.adaptedconv_transform(x.to(DEV), m.to(DEV, torch.uint8), None, packed, out=[out], sums=sums.to(DEV), tile_need=need)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("n", [33, 257, 4099])
@pytest.mark.parametrize("din", [68, 100, 128])
@pytest.mark.parametrize("D", [64, 128])
def test_need_mask_transform(D, din, n):
    """one head, 128 / 256 packed columns, inside the stream kernel's envelope: five need masks against the unmasked call"""
    x, m, head, sums, packed, g = _setup(din, D, n, seed=D + din + n)
    full = _run(x, m, sums, packed, None)                       # (h_t2s, h_s2t); need bit 0 = h_s2t, bit 1 = h_t2s
    r_s2t, r_t2s = ref_transform(x.to(DEV, torch.float64), m.to(DEV), sums.to(DEV), head)
    close(full[1][:n, :D].cpu().numpy(), r_s2t.cpu().numpy(), f"unmasked h_s2t D={D} din={din} n={n}")
    close(full[0][:n, :D].cpu().numpy(), r_t2s.cpu().numpy(), f"unmasked h_t2s D={D} din={din} n={n}")
    assert untouched(full[0][n:]) and untouched(full[1][n:])
    nt = (n + 31) // 32
    row_tile = torch.arange(n, device=DEV) // 32
    for kind in NEEDS:
        if kind == "mix":
            need = torch.randint(0, 4, (nt,), generator=g, dtype=torch.int32)
            need[:4] = torch.tensor([3, 1, 2, 0], dtype=torch.int32)[: min(4, nt)]
        else:
            need = torch.full((nt,), int(kind[3:]), dtype=torch.int32)
        need = need.to(DEV)
        got = _run(x, m, sums, packed, need)
        for table, bit, name in ((1, 0, "h_s2t"), (0, 1, "h_t2s")):
            gi, fi = got[table][:n].view(torch.int32), full[table][:n].view(torch.int32)
            same = (gi == fi).all(dim=1)                           # the whole row equals the unmasked call, bit for bit
            blank = (gi == SENTINEL).all(dim=1)                    # the whole row still holds the sentinel
            wanted = ((need[row_tile] >> bit) & 1).bool()
            assert bool(same[wanted].all()), f"{kind} {name}: {int((~same[wanted]).sum())} needed rows differ from the unmasked call"
            assert bool((same | blank)[~wanted].all()), f"{kind} {name}: a row of a tile that is not needed is neither untouched nor the unmasked row"
            assert untouched(got[table][n:]), f"{kind} {name}: guard rows written"


@pytest.mark.parametrize("din,D,n", [(36, 64, 257), (100, 31, 333)])
def test_need_mask_outside_the_stream_envelope_writes_both_tables(din, D, n):
    """Din = 36 (and a D that is no multiple of 32): another kernel runs, the mask is not honoured and both tables are written in
    full, equal to the unmasked call."""
    x, m, head, sums, packed, g = _setup(din, D, n, seed=din + D)
    full = _run(x, m, sums, packed, None)
    r_s2t, r_t2s = ref_transform(x.to(DEV, torch.float64), m.to(DEV), sums.to(DEV), head)
    close(full[1][:n, :D].cpu().numpy(), r_s2t.cpu().numpy(), f"unmasked h_s2t D={D} din={din}")
    close(full[0][:n, :D].cpu().numpy(), r_t2s.cpu().numpy(), f"unmasked h_t2s D={D} din={din}")
    nt = (n + 31) // 32
    for v in (0, 1, 2):
        got = _run(x, m, sums, packed, torch.full((nt,), v, dtype=torch.int32, device=DEV))
        for t in range(2):
            assert torch.equal(got[t].view(torch.int32), full[t].view(torch.int32)), f"need {v}, table {t}"
            assert untouched(got[t][n:])


def test_transform_entry_contract():
    """The one C entry at its own interface (N = 33, Din = 64, D = 32): the argument checks that sit in front of any launch --
    both or neither of delta_opt / sums_opt, a misaligned delta_opt, a need mask together with a tail, three team runs -- and one
    valid call per form whose tables equal those of `ops.adaptedconv_transform` bit for bit."""
    import ctypes

    from bridged_gnn_amd import _lib as L
    from bridged_gnn_amd import ops
    E_NULL, E_SHAPE, E_ALIGN = -1, -2, -4
    n, din, D = 33, 64, 32
    x, m, head, sums, packed, g = _setup(din, D, n, seed=115)
    Wp, bp, gates, _, ldh, gconst = packed
    x, m8, sums = x.to(DEV), m.to(DEV, torch.uint8), sums.to(DEV)
    delta = ops.domain_delta(sums, din)
    odd = torch.zeros(din + 4, dtype=torch.float32, device=DEV)[1:din + 1]          # 4 bytes past a 16-byte boundary
    need = torch.full(((n + 31) // 32,), 3, dtype=torch.int32, device=DEV)
    runs = (ctypes.c_int64 * 9)(0, 1, 0, 1, 2, 1, 0, 0, 0)
    small = torch.empty(2 * ldh + 2 + 8, dtype=torch.float32, device=DEV)
    lib = L.lib()

    def call(delta_t, sums_t, tails=(0, 0), need_t=None, runs_p=None, n_runs=0):
        h_t2s, h_s2t = sentinel(n + GUARD, ldh), sentinel(n + GUARD, ldh)
        rc = lib.bgnn_adaptedconv_transform_f32(
            L.ptr(x), n, din, x.stride(0), L.ptr(m8), None if delta_t is None else ctypes.c_void_p(delta_t.data_ptr()), L.ptr(sums_t),
            1, D, L.ptr(Wp), L.ptr(bp), L.ptr(gates), L.ptr(gconst), L.ptr_rows(h_s2t), L.ptr_rows(h_t2s), None, None, ldh, ldh,
            tails[0], tails[1], L.ptr(need_t), runs_p, n_runs, L.ptr(small), L.stream())
        torch.cuda.synchronize()
        return rc, h_t2s, h_s2t

    for what, want, kw in (("both delta_opt and sums_opt", E_NULL, dict(delta_t=delta, sums_t=sums)),
                           ("neither delta_opt nor sums_opt", E_NULL, dict(delta_t=None, sums_t=None)),
                           ("misaligned delta_opt", E_ALIGN, dict(delta_t=odd, sums_t=None)),
                           ("tile_need_opt with a tail", E_SHAPE, dict(delta_t=None, sums_t=sums, tails=(0, 1), need_t=need)),
                           ("n_team_runs = 3", E_SHAPE, dict(delta_t=None, sums_t=sums, runs_p=runs, n_runs=3))):
        rc, h_t2s, h_s2t = call(**kw)
        assert rc == want, f"{what}: returned {rc}, expected {want}"
        assert untouched(h_t2s) and untouched(h_s2t), f"{what}: a table was written"
    for what, kw, okw in (("delta form", dict(delta_t=delta, sums_t=None), dict(delta=delta)),
                          ("sums form", dict(delta_t=None, sums_t=sums), dict(delta=None, sums=sums))):
        rc, h_t2s, h_s2t = call(**kw)
        assert rc == 0, f"{what}: returned {rc}"
        (o_t2s, o_s2t), = ops.adaptedconv_transform(x, m8, okw.pop("delta"), packed, **okw)
        assert torch.equal(h_t2s[:n], o_t2s) and torch.equal(h_s2t[:n], o_s2t), f"{what}: tables differ from ops.adaptedconv_transform"
        assert untouched(h_t2s[n:]) and untouched(h_s2t[n:]), f"{what}: guard rows written"
