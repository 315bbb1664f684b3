"""The degree-ladder graph and the fp64 restatements that tests/test_degree_ladder_host.py and tests/test_gpu_degree_ladder.py
share.  Plain numpy / CPU torch: nothing here needs the GPU or the library.

Every aggregation kernel walks a row's edges in batches of EP * U slots (bgnn_conv_common.h: lf_ladder; bgnn_aggregate.hip:
aggregate's own switch).  The ladder graph holds, on BOTH sides of a bipartite multigraph, every degree at which such a loop can
go wrong -- 0, fewer edges than sub-groups, and k * batch - 1, k * batch, k * batch + 1 -- at every lane-group position of a
wave, so that the forward's by-destination view and the backward's by-source view are both ladders."""
import numpy as np
import torch

# ---- the tables the ladder is built for, restated (a changed kernel table fails the assertions on them, never silences them) ----
# bgnn_conv_common.h lf_ladder: float4 slots of the row (upper bound) -> (LF, EP, U)
LF_LADDER = ((1, (1, 8, 4)), (2, (2, 4, 4)), (4, (4, 2, 4)), (8, (8, 1, 8)), (16, (16, 1, 8)), (32, (32, 1, 8)))
# bgnn_aggregate.hip, aggregate()'s single-head switch: (LF, EP, U) by float4 slots; past 8 slots the wide kernels, U = 4 a lane
ADAPTED_LADDER = ((1, (1, 4, 4)), (2, (2, 2, 4)), (4, (4, 1, 8)), (8, (8, 1, 4)), (16, (16, 1, 4)), (32, (32, 1, 4)))
WIDTHS = (3, 7, 12, 31, 64, 100)          # one width per rung of lf_ladder
WIDE = 132                                # a second column slice of 4 columns (a launch covers 128)
ADAPTED_WIDTHS = (12, 31, 64, 128)        # agg_kernel (two rungs), agg_wide(_fast)_kernel at LF = 16 and 32
GAT_ALPHA_SWEEP = 8 * 4                   # gat_alpha_kernel<8, 4>: 8 lanes x 4 slots stride a row
GAT_EDGE_U = 4                            # bgnn_gat.hip launch_edge and every bgnn_gatv2.hip walk: U = 4 at every rung
GEN_BWD_U_CAP = 4                         # bgnn_gen.hip launch_bwd: gen_bwd_kernel runs at UB = min(U, 4): 4 slots at the wide rungs
SUBGROUPS = (2, 4, 8)                     # the EP values above 1
BATCHES = (4, 8, 16, 32)                  # every EP * U of the tables above
ROUNDS = (1, 2, 3)


def rung(D, table=LF_LADDER):
    """(LF, EP, U) of a slice of D <= 128 columns"""
    nv = (min(int(D), 128) + 3) // 4
    for cap, r in table:
        if nv <= cap:
            return r
    raise ValueError(D)


def rows_per_wave(D, table=LF_LADDER):
    LF, EP, _ = rung(D, table)
    return 64 // (LF * EP)


def batch_sizes():
    """every EP * U a kernel of this package walks a row with"""
    s = {EP * U for tab in (LF_LADDER, ADAPTED_LADDER) for _, (_, EP, U) in tab}
    s |= {EP * GAT_EDGE_U for _, (_, EP, _) in LF_LADDER}
    s |= {EP * min(U, GEN_BWD_U_CAP) for _, (_, EP, U) in LF_LADDER}
    s.add(GAT_ALPHA_SWEEP)
    return s


def ladder_degrees():
    d = {0, 1, 2, 3}
    for ep in SUBGROUPS:
        d |= {ep - 1, ep, ep + 1}
    for s in BATCHES:
        for k in ROUNDS:
            d |= {k * s - 1, k * s, k * s + 1}
    return sorted(d)


# ---- the graph ---------------------------------------------------------------------------------------------------------------------
VARIANTS = ("plain", "loops_dropped", "loops_rewritten")
# plain           SageGraph (SAGE, GIN, DeeperGCN): the edges as given
# loops_dropped   JKGraph: every self loop dropped, none appended
# loops_rewritten GcnGraph / GatGraph (GCN, APPNP, GCNII, GAT, GATv2): every self loop dropped, one appended per node
SEED = 20260
POSITIONS = 16


class Ladder:
    """n destinations [0, n), n sources [n, 2n); `ei` int64 [2, E]: the RAW edge list handed to the family's graph class;
    `degrees`: the ladder the WALKED view carries on both sides (without 0 where every row holds a self loop)."""

    def __init__(self, variant, seed=SEED):
        assert variant in VARIANTS
        self.variant = variant
        L = ladder_degrees()
        if variant == "loops_rewritten":
            L = [d for d in L if d >= 1]
        self.degrees = L
        m = len(L)
        # row i sits at position i % P of its run of P rows (P = 16: the most rows a wave holds, agg_kernel<4, 1, 8>; the positions
        # of 8, 4 and 2 rows per wave follow): each run holds P consecutive ladder degrees, rotated by one from run to run
        P = POSITIONS
        n = P * m + 2 * P - 3                               # m full rotations on either side behind any offset, and a ragged
        #                                                     tail: neither n nor 2n is a multiple of 8
        self.n, self.N = n, 2 * n
        i = np.arange(n)
        seq = np.asarray(L)[(i // P + i % P) % m]
        self.deg_dst = seq                                  # walked in-degree of destination i
        self.deg_src = np.roll(seq, -(n % P))               # walked out-degree of source n + i: the same multiset, rotated so that
        #                                                     the sequence sits at the same positions behind the offset n
        own = 1 if variant == "loops_rewritten" else 0      # the appended self loop is one of the walked edges
        rng = np.random.default_rng(seed)
        dst = np.repeat(i, self.deg_dst - own)
        src = np.repeat(n + i, self.deg_src - own)
        src = src[rng.permutation(src.shape[0])]
        ei = np.stack((src, dst)).astype(np.int64)
        if variant != "plain":                              # raw self loops the graph class has to drop (some twice on one node)
            loops = np.concatenate((np.arange(0, self.N, 7), np.arange(0, self.N, 21)))
            ei = np.concatenate((ei, np.stack((loops, loops))), axis=1)
            ei = ei[:, rng.permutation(ei.shape[1])]
        self.ei = ei

    def walked(self):
        """(src, dst) int64 of the edges the family's graph class keeps, in by-destination order (stable), restated on the CPU"""
        src, dst = self.ei
        if self.variant != "plain":
            keep = src != dst
            src, dst = src[keep], dst[keep]
        if self.variant == "loops_rewritten":
            a = np.arange(self.N)
            src, dst = np.concatenate((src, a)), np.concatenate((dst, a))
        o = np.argsort(dst, kind="stable")
        return src[o], dst[o]

    def duplicates(self):
        src, dst = self.walked()
        key = src * self.N + dst
        return key.shape[0] - np.unique(key).shape[0]


def csr_by(rows, cols, N):
    """CSR over `rows` (stable): (rowptr int64 [N + 1], col int64 [E])"""
    o = np.argsort(rows, kind="stable")
    rowptr = np.zeros(N + 1, np.int64)
    rowptr[1:] = np.cumsum(np.bincount(rows, minlength=N))
    return rowptr, cols[o]


def coverage(rowptr, rpw, heads=1):
    """{degree: set of lane-group positions at which a row of that degree occurs} of a view of rowptr [rows + 1].  A lane group owns
    row i at position i % rpw; with `heads` > 1 (the attention kernels) it owns the VIRTUAL row v = i * heads + h, at v % rpw."""
    rowptr = np.asarray(rowptr, np.int64)
    deg = np.repeat(rowptr[1:] - rowptr[:-1], heads)
    pos = np.arange(deg.shape[0]) % rpw
    out = {}
    for d, p in zip(deg.tolist(), pos.tolist()):
        out.setdefault(d, set()).add(p)
    return out


def assert_coverage(rowptr, degrees, rpw, what, heads=1):
    """every ladder degree at every lane-group position of the view; -> the degrees seen (named in the failure message)"""
    cov = coverage(rowptr, rpw, heads)
    missing = [(d, sorted(set(range(rpw)) - cov.get(d, set()))) for d in degrees if cov.get(d, set()) != set(range(rpw))]
    assert not missing, f"{what}: ladder degrees without every position of {rpw} rows per wave: {missing}; degrees seen {sorted(cov)}"
    return sorted(cov)


def assert_batches_bracketed(degrees, what="ladder"):
    """the ladder brackets every batch size of the restated tables, and holds a degree below every sub-group count"""
    ds = set(degrees)
    for s in sorted(batch_sizes()):
        need = {k * s + o for k in ROUNDS for o in (-1, 0, 1)}
        assert need <= ds, f"{what}: batch of {s} slots is not bracketed: {sorted(need - ds)} missing"
    for ep in SUBGROUPS:
        assert {ep - 1, ep, ep + 1} <= ds, f"{what}: EP = {ep}"
    assert 1 in ds and 2 in ds and 3 in ds


# ---- fp64 restatements over a CSR (rowptr, col): CPU torch, the same fp32 inputs as the kernel -----------------------------------
def _edges(rowptr, col):
    rowptr = torch.as_tensor(rowptr).long()
    deg = rowptr[1:] - rowptr[:-1]
    return torch.repeat_interleave(torch.arange(deg.shape[0]), deg), torch.as_tensor(col).long()[: int(rowptr[-1])]


def walk(rowptr, col, X, w=None):
    """S_i = sum_{t in row i} w_t X[col[t]] and A_i = sum |w_t X[col[t]]| in fp64 ([rows, D] each); w: per-edge weights or None"""
    dst, src = _edges(rowptr, col)
    X = X.double()
    v = X[src] if w is None else X[src] * w.double()[:, None]
    rows = int(torch.as_tensor(rowptr).shape[0]) - 1
    z = torch.zeros(rows, X.shape[1], dtype=torch.float64)
    return z.index_add(0, dst, v), z.index_add(0, dst, v.abs())


def row_scale(A):
    """a row's scale: its largest column of sum |coefficient * value|"""
    return A.abs().max(dim=1).values


def sage_ref(rowptr, col, T, root=None, mean=True):
    S, A = walk(rowptr, col, T)
    rp = torch.as_tensor(rowptr).long()
    deg = (rp[1:] - rp[:-1]).double()
    s = torch.where(deg > 0, 1.0 / deg.clamp(min=1), torch.zeros_like(deg)) if mean else torch.ones_like(deg)
    out, ab = S * s[:, None], A * s[:, None]
    if root is not None:
        out, ab = out + root.double(), ab + root.double().abs()
    return out, ab


def scaled_ref(rowptr, col, T, s_row, s_col, own=None, w_own=None, bias=None):
    """out_i = w_own_i * own_i + s_row_i * sum_t s_col[col[t]] * T[col[t]] + bias -- GCN (s = dinv, no own term), JKNet (s, w),
    GIN (s = 1, w_own = 1 + eps) and one APPNP step are all this"""
    dst, src = _edges(rowptr, col)
    S, A = walk(rowptr, col, T, s_col.double()[src])
    rows = S.shape[0]
    out, ab = S * s_row.double()[:rows, None], A * s_row.double().abs()[:rows, None]
    if own is not None:
        o = own.double()[:rows] * (w_own.double()[:rows, None] if torch.is_tensor(w_own) and w_own.dim() == 1 else float(w_own))
        out, ab = out + o, ab + o.abs()
    if bias is not None:
        out, ab = out + bias.double(), ab + bias.double().abs()
    return out, ab


def appnp_ref(rowptr, col, h, dinv, K, alpha):
    """z_0 = h, z_{k+1} = (1 - alpha) A^ z_k + alpha h -> (z_K, its row scale matrix: the same recurrence on absolute values)"""
    z, a = h.double(), h.double().abs()
    for _ in range(int(K)):
        zs, _ = scaled_ref(rowptr, col, z, dinv, dinv)
        as_, _ = scaled_ref(rowptr, col, a, dinv, dinv)
        z, a = (1 - alpha) * zs + alpha * h.double(), (1 - alpha) * as_ + alpha * h.double().abs()
    return z, a


def gcn2_ref(rowptr, col, x, x0, M, dinv, alpha):
    """m = (1 - alpha) A^ x + alpha x0, out = relu(m @ M) -> (out, m, scale matrix of out, scale matrix of m)"""
    s, a = scaled_ref(rowptr, col, x, dinv, dinv)
    m, ma = (1 - alpha) * s + alpha * x0.double(), (1 - alpha) * a + alpha * x0.double().abs()
    return torch.relu(m @ M.double()), m, ma @ M.double().abs(), ma


def gen_ref(rowptr, col, x, t):
    """DeeperGCN's softmax aggregation per channel: v = relu(x) + 1e-7, z_i = sum_j softmax_j(t v_j) v_j + x_i ->
    (z, lse, o, scale matrix of z); a row without edges: z = x, lse = o = 0"""
    dst, src = _edges(rowptr, col)
    x = x.double()
    rows = int(torch.as_tensor(rowptr).shape[0]) - 1
    v = torch.relu(x) + 1e-7
    e = float(t) * v[src]
    mx = torch.full((rows, x.shape[1]), -float("inf"), dtype=torch.float64).index_reduce(0, dst, e, "amax", include_self=True)
    has = torch.isfinite(mx)
    mx0 = torch.where(has, mx, torch.zeros_like(mx))
    p = torch.exp(e - mx0[dst])
    den = torch.zeros(rows, x.shape[1], dtype=torch.float64).index_add(0, dst, p)
    a = p / den[dst]
    o = torch.zeros(rows, x.shape[1], dtype=torch.float64).index_add(0, dst, a * v[src])
    lse = torch.where(has, mx0 + torch.log(den.clamp(min=1e-300)), torch.zeros_like(mx0))
    return o + x[:rows], lse, o, o.abs() + x[:rows].abs()


def gen_bwd_ref(rowptr, col, x, gz, t):
    """(grad_x, grad_t, scale matrix of grad_x) of gen_ref's z under the output gradient gz, written out edge by edge:
    dv_j = sum_i a_ij g_i (1 + t (v_j - o_i)), grad_x_j = [x_j > 0] dv_j + g_j, grad_t = sum a g (v_j - o_i) v_j; the fourth result
    is grad_t's scale, the sum of |a g (v_j - o_i) v_j| over every edge and channel"""
    dst, src = _edges(rowptr, col)
    x, gz = x.double(), gz.double()
    n_src = x.shape[0]
    _, lse, o, _ = gen_ref(rowptr, col, x, t)
    v = torch.relu(x) + 1e-7
    a = torch.exp(float(t) * v[src] - lse[dst])
    c = a * gz[dst] * (1 + float(t) * (v[src] - o[dst]))
    z = torch.zeros(n_src, x.shape[1], dtype=torch.float64)
    dv, dva = z.index_add(0, src, c), z.index_add(0, src, c.abs())
    pos = (x > 0).double()
    g_own = torch.zeros_like(x)
    g_own[: gz.shape[0]] = gz
    gte = a * gz[dst] * (v[src] - o[dst]) * v[src]
    return pos * dv + g_own, gte.sum(), pos * dva + g_own.abs(), gte.abs().sum()


def gen_lse_scale(rowptr, col, x, t):
    """the scale of lse_i = max_j (t v_j) + log sum_j exp(t v_j - max) per row and channel: max_j |t v_j| over the row's own
    neighbours plus log(deg_i); 0 for a row without edges"""
    dst, src = _edges(rowptr, col)
    rows = int(torch.as_tensor(rowptr).shape[0]) - 1
    v = torch.relu(x.double()) + 1e-7
    mx = torch.zeros(rows, x.shape[1], dtype=torch.float64).index_reduce(0, dst, (float(t) * v[src]).abs(), "amax", include_self=True)
    rp = torch.as_tensor(rowptr).long()
    deg = (rp[1:] - rp[:-1]).double()
    return mx + torch.log(deg.clamp(min=1))[:, None]


def gat_ref(rowptr, col, T, att_src, att_dst, H, C, slope, gy=None):
    """GAT over a CSR: -> dict(out, out_abs, s_src, s_dst, alpha [E, H]) and, with gy, the backward edge by edge as bgnn_gat.hip
    states it: grad_tbl (the gather part) with its scale matrix, ds_src, ds_dst with theirs"""
    dst, src = _edges(rowptr, col)
    rows = int(torch.as_tensor(rowptr).shape[0]) - 1
    Tv = T.double()[:, : H * C].reshape(-1, H, C)
    s_src = (Tv * att_src.double().reshape(1, H, C)).sum(-1)
    s_dst = (Tv * att_dst.double().reshape(1, H, C)).sum(-1)
    z = s_src[src] + s_dst[dst]
    e = torch.where(z > 0, z, slope * z)
    mx = torch.full((rows, H), -float("inf"), dtype=torch.float64).index_reduce(0, dst, e, "amax", include_self=True)
    p = torch.exp(e - mx[dst])
    den = torch.zeros(rows, H, dtype=torch.float64).index_add(0, dst, p)
    al = p / den[dst]
    msg = al[:, :, None] * Tv[src]
    zz = torch.zeros(rows, H, C, dtype=torch.float64)
    r = dict(out=zz.index_add(0, dst, msg).reshape(rows, H * C), out_abs=zz.index_add(0, dst, msg.abs()).reshape(rows, H * C),
             s_src=s_src, s_dst=s_dst, alpha=al)
    if gy is not None:
        g = gy.double()[:, : H * C].reshape(-1, H, C)
        N = Tv.shape[0]
        gm = al[:, :, None] * g[dst]
        zs = torch.zeros(N, H, C, dtype=torch.float64)
        r["grad_tbl"], r["grad_tbl_abs"] = zs.index_add(0, src, gm).reshape(N, H * C), zs.index_add(0, src, gm.abs()).reshape(N, H * C)
        dot = (g[dst] * Tv[src]).sum(-1)
        rr = torch.zeros(rows, H, dtype=torch.float64).index_add(0, dst, al * dot)
        dz = al * (dot - rr[dst]) * torch.where(z > 0, torch.ones_like(z), torch.full_like(z, slope))
        # a dz term is alpha * (dot - r), dot = sum_c g T and r = sum_t alpha_t dot_t: its scale is alpha * (D + sum_t alpha_t D_t)
        # with D = sum_c |g T| -- absolute values term by term, so that a dot product that cancels keeps the scale of its terms
        # (a row of one edge has dot - r = 0 exactly, and the kernel's two roundings of the same dot product do not cancel)
        dota = (g[dst].abs() * Tv[src].abs()).sum(-1)
        ra = torch.zeros(rows, H, dtype=torch.float64).index_add(0, dst, al * dota)
        dza = al * (dota + ra[dst])
        r["ds_src"], r["ds_src_abs"] = torch.zeros(N, H, dtype=torch.float64).index_add(0, src, dz), torch.zeros(N, H, dtype=torch.float64).index_add(0, src, dza)
        r["ds_dst"], r["ds_dst_abs"] = torch.zeros(rows, H, dtype=torch.float64).index_add(0, dst, dz), torch.zeros(rows, H, dtype=torch.float64).index_add(0, dst, dza)
    return r


def gatv2_ref(rowptr, col, XL, XR, att, H, C, slope, gy=None):
    """GATv2 over a CSR: e = <att, leaky(x_l[j] + x_r[i])> per head -> dict(out, out_abs, alpha) and, with gy, (dxl, dxr, datt) with
    the scale matrices of dxl and dxr, edge by edge"""
    dst, src = _edges(rowptr, col)
    rows = int(torch.as_tensor(rowptr).shape[0]) - 1
    xl, xr = XL.double()[:, : H * C].reshape(-1, H, C), XR.double()[:, : H * C].reshape(-1, H, C)
    a = att.double().reshape(1, H, C)
    u = xl[src] + xr[dst]
    lu = torch.where(u > 0, u, slope * u)
    e = (lu * a).sum(-1)
    mx = torch.full((rows, H), -float("inf"), dtype=torch.float64).index_reduce(0, dst, e, "amax", include_self=True)
    p = torch.exp(e - mx[dst])
    den = torch.zeros(rows, H, dtype=torch.float64).index_add(0, dst, p)
    al = p / den[dst]
    msg = al[:, :, None] * xl[src]
    zz = torch.zeros(rows, H, C, dtype=torch.float64)
    r = dict(out=zz.index_add(0, dst, msg).reshape(rows, H * C), out_abs=zz.index_add(0, dst, msg.abs()).reshape(rows, H * C), alpha=al)
    if gy is not None:
        g = gy.double()[:, : H * C].reshape(-1, H, C)
        N = xl.shape[0]
        dot = (g[dst] * xl[src]).sum(-1)
        rr = torch.zeros(rows, H, dtype=torch.float64).index_add(0, dst, al * dot)
        dota = (g[dst].abs() * xl[src].abs()).sum(-1)                             # term by term, as in gat_ref
        ra = torch.zeros(rows, H, dtype=torch.float64).index_add(0, dst, al * dota)
        de, dea = al * (dot - rr[dst]), al * (dota + ra[dst])
        slp = torch.where(u > 0, torch.ones_like(u), torch.full_like(u, slope))
        du, dua = de[:, :, None] * a * slp, dea[:, :, None] * a.abs() * slp
        gm = al[:, :, None] * g[dst]
        zs = torch.zeros(N, H, C, dtype=torch.float64)
        r["dxl"], r["dxl_abs"] = zs.index_add(0, src, gm + du).reshape(N, H * C), zs.index_add(0, src, gm.abs() + dua).reshape(N, H * C)
        r["dxr"], r["dxr_abs"] = zz.index_add(0, dst, du).reshape(rows, H * C), zz.index_add(0, dst, dua).reshape(rows, H * C)
        r["datt"], r["datt_abs"] = (de[:, :, None] * lu).sum(0).reshape(-1), (dea[:, :, None] * lu.abs()).sum(0).reshape(-1)
    return r


def adapted_ref(rowptr, col, hS, hT, a1, a2, mask, D, slope, gout=None):
    """The single-head AdaptedConv aggregation (KTGNN.py:292-305 as bgnn_aggregate.hip fuses it): a destination i of the source
    domain (mask[i]) reads table h_t2s = hS and attention vector a1, a target-domain destination reads hT and a2;
    e_t = <a, leaky(h[col[t]] + h[i])>, out_i = sum_t softmax_t(e) h[col[t]] -> dict(out, out_abs, alpha [E]) and, with gout, the
    gradients of both tables and both vectors through torch autograd in fp64, with an edge-by-edge scale of the tables' rows."""
    dst, src = _edges(rowptr, col)
    rows = int(torch.as_tensor(rowptr).shape[0]) - 1
    m = torch.as_tensor(mask).bool()[:rows]
    tS, tT = hS.double()[:, :D].clone().requires_grad_(gout is not None), hT.double()[:, :D].clone().requires_grad_(gout is not None)
    b1, b2 = a1.double()[:D].clone().requires_grad_(gout is not None), a2.double()[:D].clone().requires_grad_(gout is not None)
    md = m[dst][:, None]
    hj = torch.where(md, tS[src], tT[src])
    hi = torch.where(md, tS[dst], tT[dst])
    av = torch.where(md, b1[None, :], b2[None, :])
    e = (torch.nn.functional.leaky_relu(hj + hi, slope) * av).sum(-1)
    mx = torch.full((rows,), -float("inf"), dtype=torch.float64).index_reduce(0, dst, e.detach(), "amax", include_self=True)
    p = torch.exp(e - mx[dst])
    den = torch.zeros(rows, dtype=torch.float64).index_add(0, dst, p)
    al = p / den[dst]
    msg = al[:, None] * hj
    zz = torch.zeros(rows, D, dtype=torch.float64)
    out = zz.index_add(0, dst, msg)
    r = dict(out=out.detach(), out_abs=zz.index_add(0, dst, msg.detach().abs()), alpha=al.detach())
    if gout is not None:
        g = gout.double()[:rows, :D]
        (out * g).sum().backward()
        r["grads"] = (tS.grad, tT.grad, b1.grad, b2.grad)
        # scale of a table row: what the gather adds (alpha |g_i|) and the logit terms |de| |a| on both ends of every edge
        with torch.no_grad():
            ald, hjd = al.detach(), hj.detach()
            dota = (g[dst].abs() * hjd.abs()).sum(-1)                             # term by term, as in gat_ref
            ra = torch.zeros(rows, dtype=torch.float64).index_add(0, dst, ald * dota)
            dea = (ald * (dota + ra[dst]))[:, None] * av.detach().abs()
            N = tS.shape[0]
            zs = torch.zeros(N, D, dtype=torch.float64)
            sc = zs.index_add(0, src, ald[:, None] * g[dst].abs() + dea).index_add(0, dst, dea)
            r["grads_abs"] = sc
    return r


def dense_counts(rowptr, col, n_cols):
    """A[i, j] = number of edges j -> i of the view, fp64 [rows, n_cols]"""
    dst, src = _edges(rowptr, col)
    rows = int(torch.as_tensor(rowptr).shape[0]) - 1
    A = torch.zeros(rows * n_cols, dtype=torch.float64)
    A.index_add_(0, dst * n_cols + src, torch.ones(dst.shape[0], dtype=torch.float64))
    return A.reshape(rows, n_cols)


# ---- judging a result row by row --------------------------------------------------------------------------------------------------
def judge(got, ref, scale_mat, bar, deg, what):
    """every row of `got` within bar * (that row's own scale) of `ref`; -> (worst share of the bar, the degree of that row).
    scale_mat: sum |coefficient * value| per element (its largest column is the row's scale).  A row whose scale is 0 must be
    exactly its reference."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite entries"
    err = (got - ref).abs().reshape(got.shape[0], -1).max(dim=1).values
    sc = row_scale(scale_mat.reshape(got.shape[0], -1))
    tol = bar * sc
    bad = torch.nonzero(err > tol).reshape(-1)
    deg = torch.as_tensor(np.asarray(deg)).long()
    share = torch.where(sc > 0, err / (bar * sc).clamp(min=1e-300), torch.zeros_like(err))
    w = int(torch.argmax(share))
    if bad.numel():
        i = int(bad[torch.argmax(share[bad])]) if bool((sc[bad] > 0).any()) else int(bad[0])
        raise AssertionError(f"{what}: {bad.numel()} rows beyond {bar:g} of their own scale; worst row {i} (degree {int(deg[i])}): "
                             f"error {err[i].item():.3e}, scale {sc[i].item():.3e}, share {share[i].item():.2f}; degrees of the failing "
                             f"rows {sorted(set(deg[bad].tolist()))}")
    return share[w].item(), int(deg[w])
