"""GPU: the need-mask transform (bgnn_adaptedconv_transform_need_f32, `ops.adaptedconv_transform(..., tile_need=...)`) at its own
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
