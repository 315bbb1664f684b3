"""GPU: the pipelined kernels of csrc/bgnn_gram.hip -- the Gram product behind every weight gradient (`ops.gram`), `ops.rowdot`
and `ops.transform_bwd_prep` -- at sizes where every block runs its loops past the first pass, against exact integer
arithmetic or fp64 torch on the device.

What the shapes reach (tests/test_gpu_training.py stops at one 32-row slice per block and one row per lane group):
  * Gram: R rows per block for R in R_SWEEP = 3..11 sixteen-row tiles of the bf16x3 kernel (0..3 turns of the staging waves'
    steady loop, both register sets, both LDS buffers reused, odd and even tile counts, full and one-row last tiles) and
    2..6 tiles of the fp32 kernel; every row-block count 1..9 (P_SWEEP) and 1..4 multiplying waves (Q_SWEEP).  The block
    count comes from the public entry (`_blocks`), so the sizes follow the library if its grid changes.  Each R is run with
    every block full (N = blocks R) and with a partial last block followed by blocks that own no rows
    (N = blocks (R - 1) + 1).
  * rowdot: second and third passes under the grid cap (N > 65536), nv = 3.
  * transform_bwd_prep: the four-rows-in-flight loop on every route (N > 3 x the rows of one pass).

How they are pinned:
  1. integer operands (|x| <= 8): every bf16 piece, product and partial sum is exact, the result must EQUAL the integer
     product -- a dropped, doubled or stale tile cannot survive.
  2. probes: one full-mantissa product per output element; per element |err| <= PROBE_BAR 2^-24 |exact|.  In a CPU emulation
     of the six kept piece products (2M pairs) the full sum is within 1.65 x 2^-24; without lo*hi, hi*lo or mid*mid the
     error is above 16 x 2^-24 on 60% of the pairs (up to 128 x), without mid*hi or hi*mid it is ~1e-3 -- and a case here
     takes the maximum over at least 144 elements.
  3. dense normal operands: the derived per-element worst case of an fp32 accumulation, and exact power-of-two column
     scaling (which pins columns of size 1/N next to O(1) ones without a tolerance).
  4. rowdot: exact on integers, d 2^-24 |X| |V|^T on floats.
  5. prep: the fp64 restatement and bars of test_transform_bwd_prep_matches_torch_formula, plus bit-equality of the rows
     of a large call with the rows of 4096-row calls (which take the one-row loop).

Measured on an MI355X: 54 tests (364 + 64 + 30 integer Gram shapes, 72 probe and 12 dense ones, 144 rowdot shapes, 5 prep
cases), 5 s for the file.  Worst figures over the cases (bars in brackets):
  probe |err| / |exact|: 2.56 x 2^-24 on the bf16x3 kernel (p = 132; 2.28 .. 2.56 over its p), 0.99 x 2^-24 on the fp32 kernel  [4]
  dense err / bound: 3e-4 (err / S <= 8.0e-9 where torch's own fp32 A^T B has 1.3e-7); the +-1/N column alone 1e-4    [1]
  rowdot err / bound: 0.72 at d = 4, 0.06 at d = 36, 0.004 at d = 256                                                  [1]
  prep: rows of the four-row loop bit-equal to those of the one-row loop on every route.
Altered on purpose in scratch builds, one at a time: the stager's steady loop storing register set A where B belongs fails
every integer, slice, probe and dense case of the bf16x3 kernel with 5 or more tiles per block and none with fewer;
without the lo*hi MFMA only the probes fail (117 .. 124 x 2^-24); the four-row loop of the prep kernel finishing every row
from the first row's registers fails all five prep cases here.  tests/test_gpu_training.py passes all three.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

U = 2.0 ** -24                                                   # unit roundoff of fp32
R_SWEEP = (33, 47, 48, 49, 64, 65, 80, 81, 96, 97, 128, 129, 161)
P_SWEEP = (4, 8, 32, 36, 68, 96, 128, 132, 164, 192, 224, 256, 260, 288)
Q_SWEEP = (4, 36, 100, 128)
PROBE_BAR = 4.0                                                  # units of 2^-24 |exact|; never above 16 (a lost lo*hi term: up to 128)


def _blocks(p, q):
    """persistent blocks of a Gram launch, from the public workspace size: one [p][q] fp32 partial per block + 256 bytes"""
    from bridged_gnn_amd import _lib
    return (int(_lib.lib().bgnn_gram_workspace_bytes(p, q)) - 256) // (4 * p * q)


def _sizes(p, q, R):
    """(N with every block full, N with a one-row last block and trailing blocks without rows); R rows per block in both"""
    nb = _blocks(p, q)
    return nb * R, nb * (R - 1) + 1


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _ints(g, n, c, k):
    return torch.randint(-k, k + 1, (n, c), device=DEV, generator=g).float()


def _exact_gram(A, B):
    return A.double().t() @ B.double()                           # integers: every fp64 partial sum is exact


def _gram_twice_equals(A, B, ref):
    from bridged_gnn_amd import ops
    got, again = ops.gram(A, B), ops.gram(A, B)
    return torch.equal(got.double(), ref), torch.equal(got, again)


def test_block_counts_put_the_sweep_where_it_is_meant_to_be():
    """the sizes below rest on these: the launch uses all `blocks` only if N > 32 (blocks - 1), a block then owns R rows, and
    the exact-integer argument needs 64 N < 2^24"""
    for p in P_SWEEP:
        for q in Q_SWEEP:
            nb = _blocks(p, q)
            assert nb >= 1
            for R in R_SWEEP:
                for N in _sizes(p, q, R):
                    assert (N + 31) // 32 >= nb and -(-N // nb) == R and 64 * N < 2 ** 24


@pytest.mark.parametrize("p", P_SWEEP)
def test_gram_of_integers_is_exact_for_3_to_11_tiles_per_block(p):
    ip = P_SWEEP.index(p)
    g = _gen(1000 + p)
    nmax = max(_blocks(p, q) for q in Q_SWEEP) * max(R_SWEEP)
    Amax, Bmax = _ints(g, nmax, p, 8), _ints(g, nmax, 128, 8)
    wrong, unstable, ncase = [], [], 0
    for iR, R in enumerate(R_SWEEP):
        for full in (0, 1):
            q = Q_SWEEP[(ip + iR + 2 * full) % 4]                # every q meets every R over the p sweep (and over 4 R in a row)
            N = _sizes(p, q, R)[full]
            lo = (iR * 7919) % (nmax - N + 1)                    # another window of the data for every case
            A, B = Amax[lo:lo + N], Bmax[lo:lo + N, :q].contiguous()
            ok, same = _gram_twice_equals(A, B, _exact_gram(A, B))
            ncase += 1
            if not ok:
                wrong.append((p, q, R, N))
            if not same:
                unstable.append((p, q, R, N))
    assert ncase == 2 * len(R_SWEEP)
    assert not wrong and not unstable, f"(p, q, rows per block, N) not exact: {wrong}; two calls differ: {unstable}"


@pytest.mark.parametrize("p", (8, 36, 132, 288))
def test_gram_of_integers_is_exact_for_a_handful_of_rows(p):
    """N = 0 (no rows: all zeros), one row, and one row either side of the 16- and 32-row tiles"""
    g = _gen(2000 + p)
    wrong = []
    for q in (4, 100):
        for N in (0, 1, 15, 16, 17, 31, 32, 33):
            A, B = _ints(g, N, p, 8), _ints(g, N, q, 8)
            ok, same = _gram_twice_equals(A, B, _exact_gram(A, B))
            if not (ok and same):
                wrong.append((p, q, N))
    assert not wrong, wrong


@pytest.mark.parametrize("p,q,R", [(8, 36, 65), (36, 128, 81), (132, 100, 97), (164, 4, 80), (260, 128, 129), (288, 36, 161)])
def test_gram_of_integers_through_column_slices(p, q, R):
    """A and B as column slices of wider buffers (lda > p, ldb > q; NaN in the columns that are not operands), and A as the
    second half of a [N, 2p] buffer: a read outside the operand's columns turns the result into NaN."""
    g = _gen(3000 + p + R)
    wrong = []
    for N in _sizes(p, q, R):
        bufA = torch.full((N, p + 12), float("nan"), device=DEV)
        bufB = torch.full((N, q + 8), float("nan"), device=DEV)
        A, B = bufA[:, 8:8 + p], bufB[:, 4:4 + q]
        A.copy_(_ints(g, N, p, 8)); B.copy_(_ints(g, N, q, 8))
        assert A.stride(0) == p + 12 and B.stride(0) == q + 8
        if _gram_twice_equals(A, B, _exact_gram(A, B)) != (True, True):
            wrong.append(("slices", N))
        pair = torch.full((N, 2 * p), float("nan"), device=DEV)
        A2 = pair[:, p:]
        A2.copy_(_ints(g, N, p, 8))
        if _gram_twice_equals(A2, B, _exact_gram(A2, B)) != (True, True):
            wrong.append(("second half", N))
    assert not wrong, wrong


@pytest.mark.parametrize("R", (49, 97, 161))
def test_gram_of_a_side_table_against_a_column_block_of_gall(R):
    """the call of _TransformFn.backward for D > 128: A = side [N, 4], B = Gall[:, 128:256] of a [N, 264] buffer"""
    g = _gen(4000 + R)
    wrong = []
    for N in _sizes(4, 128, R):
        Gall = torch.full((N, 264), float("nan"), device=DEV)
        B = Gall[:, 128:256]
        B.copy_(_ints(g, N, 128, 8))
        side = _ints(g, N, 4, 8)
        if _gram_twice_equals(side, B, _exact_gram(side, B)) != (True, True):
            wrong.append(N)
    assert not wrong, wrong


# ---- 2. one full-mantissa product per output element

def _wide_range(g, shape):
    """sign x lognormal magnitude in [1e-6, 1e6]: all 24 significand bits in use, so the mid and lo bf16 pieces are non-zero"""
    mag = torch.exp(3.0 * torch.randn(shape, device=DEV, generator=g, dtype=torch.float64)).clamp(1e-6, 1e6).float()
    sign = torch.randint(0, 2, shape, device=DEV, generator=g).float() * 2 - 1
    return mag * sign


@pytest.mark.parametrize("p", (8, 36, 96, 132, 260, 288))
def test_gram_probes_carry_one_product_to_fp32_accuracy(p):
    """A is zero but for one entry per column, in distinct rows drawn uniformly from [0, N): out[a][b] = A[r_a, a] B[r_a, b],
    one product that travels through whichever block, tile, LDS buffer and register set row r_a falls in.  The bf16x3
    kernel keeps six of the nine piece products (an emulation -- three bf16 roundings, smallest terms first, fp32
    accumulation -- gives <= 1.65 x 2^-24 over 2M pairs; what the MFMA adds to that is measured here: module docstring);
    the fp32 kernel (p = 8) rounds the product once."""
    from bridged_gnn_amd import ops
    ip = (8, 36, 96, 132, 260, 288).index(p)
    worst, over = 0.0, []
    for iR, R in enumerate((49, 81, 129)):
        for seed in range(4):
            q = Q_SWEEP[(ip + iR + seed) % 4]
            N = _sizes(p, q, R)[seed & 1]
            g = _gen(5000 + 100 * p + 10 * R + seed)
            B = _wide_range(g, (N, q))
            rows = torch.randperm(N, device=DEV, generator=g)[:p]
            vals = _wide_range(g, (p,))
            A = torch.zeros(N, p, device=DEV)
            A[rows, torch.arange(p, device=DEV)] = vals
            exact = vals.double()[:, None] * B[rows].double()                    # 48-bit products: exact in fp64
            got = ops.gram(A, B).double()
            ratio = float(((got - exact).abs() / exact.abs()).max()) / U
            worst = max(worst, ratio)
            if not ratio <= PROBE_BAR:
                over.append((p, q, R, N, seed, round(ratio, 2)))
    print(f"\nGRAMSTAT probe p={p}: worst |err| / |exact| = {worst:.3f} x 2^-24 (bar {PROBE_BAR})")
    assert not over, f"(p, q, rows per block, N, seed, ratio in 2^-24): {over}"


# ---- 3. dense normal operands

@pytest.mark.parametrize("q", (36, 128))
@pytest.mark.parametrize("p", (8, 128, 260))
def test_gram_of_normal_operands_per_element_bound_and_exact_column_scaling(p, q):
    """Per element |got - ref64| <= (6 R + 8) 2^-24 1.02 S, S = |A|^T |B|: a block accumulates the 6 R exact piece products
    of an element in fp32 in some order (worst case (6 R - 1) u S to first order; 1.02 covers the higher orders), the
    dropped terms are < 2 u S, the sum over blocks is fp64 and the final rounding is u -- derived, not measured.
    Then the same call with column a of A times 2^k_a and column b of B times 2^m_b must give the first result times
    2^(k_a + m_b) bit for bit: a power of two commutes with every rounding of both kernels.  Columns: one of A is +-1/N (as
    column 2D+2 of Gall), one of A and one of B are zero (Gall's padding) and must give exact zeros."""
    from bridged_gnn_amd import ops
    rng = np.random.default_rng(p + q)
    for R in (81, 161):
        N = _blocks(p, q) * R
        g = _gen(6000 + p + q + R)
        A, B = torch.randn(N, p, device=DEV, generator=g), torch.randn(N, q, device=DEV, generator=g)
        A[:, 1] = 0.0
        A[:, 2] = (torch.randint(0, 2, (N,), device=DEV, generator=g).float() * 2 - 1) / N
        B[:, 3] = 0.0
        got = ops.gram(A, B)
        A64, B64 = A.double(), B.double()
        ref, S = A64.t() @ B64, A64.abs().t() @ B64.abs()
        err = (got.double() - ref).abs()
        bound = (6 * R + 8) * U * 1.02 * S
        live = S > 0
        mine, lib = float((err[live] / S[live]).max()), float((((A.t() @ B).double() - ref).abs()[live] / S[live]).max())
        print(f"\nGRAMSTAT dense p={p} q={q} R={R} N={N}: worst err / S = {mine:.3e} (torch fp32 matmul {lib:.3e}); "
              f"worst err / bound = {float((err[live] / bound[live]).max()):.4f}; column +-1/N alone: "
              f"{float((err[2] / bound[2].clamp_min(1e-300)).max()):.4f}")
        assert bool((err <= bound).all()), (p, q, R, float((err[live] / bound[live]).max()))
        assert float(got[1].abs().max()) == 0.0 and float(got[:, 3].abs().max()) == 0.0
        ka, mb = rng.integers(-20, 21, size=p), rng.integers(-20, 21, size=q)
        sa = torch.from_numpy(np.ldexp(1.0, ka).astype(np.float32)).to(DEV)       # exact powers of two
        sb = torch.from_numpy(np.ldexp(1.0, mb).astype(np.float32)).to(DEV)
        scaled = ops.gram(A * sa, B * sb)
        assert torch.equal(scaled, got * sa[:, None] * sb[None, :]), (p, q, R)


# ---- 4. rowdot

def _rowdot(X, V):
    """ops.rowdot with a row-strided V (the wrapper asks for a contiguous one)"""
    from bridged_gnn_amd import _lib as L
    out = torch.empty(X.shape[0], V.shape[0], dtype=torch.float32, device=X.device)
    rc = L.lib().bgnn_rowdot_f32(L.ptr_rows(X), X.stride(0), X.shape[0], X.shape[1], L.ptr_rows(V), V.stride(0), V.shape[0],
                                 L.ptr(out), L.stream())
    L.check(rc, "bgnn_rowdot_f32")
    return out


@pytest.mark.parametrize("d", (4, 36, 64, 68, 128, 132, 192, 252, 256))
def test_rowdot_beyond_one_pass_exact_on_integers_and_bounded_on_floats(d):
    """N > 65536 = 4096 blocks x 16 rows: blocks take a second and a third pass; nv = 1..4; X a column slice (row stride
    d + 4), V with row stride d + 8, NaN in the columns outside.  Integers in [-16, 16]: |sum| <= 2^16, exact.  Floats:
    |err| <= d 2^-24 |X| |V|^T, the worst case of a sum of d products in any order."""
    from bridged_gnn_amd import ops
    g = _gen(7000 + d)
    nmax = 2 * 65536 + 5
    assert nmax > 2 * 4096 * 16                                              # bgnn_rowdot_f32: grid > 4096 ? 4096 blocks of 16 rows
    bufI = torch.full((nmax, d + 4), float("nan"), device=DEV)
    bufF = torch.full((nmax, d + 4), float("nan"), device=DEV)
    bufI[:, :d] = _ints(g, nmax, d, 16)
    bufF[:, :d] = torch.randn(nmax, d, device=DEV, generator=g)
    wrong, worst = [], 0.0
    for nv in (1, 2, 3, 4):
        VI = torch.full((nv, d + 8), float("nan"), device=DEV)
        VF = torch.full((nv, d + 8), float("nan"), device=DEV)
        VI[:, :d] = _ints(g, nv, d, 16)
        VF[:, :d] = torch.randn(nv, d, device=DEV, generator=g)
        for N in (3, 65536, 65536 + 17, 2 * 65536 + 5):
            XI, XF = bufI[nmax - N:, :d], bufF[nmax - N:, :d]                # (the last N rows: every size sees other data)
            assert XI.stride(0) == d + 4 and VI[:, :d].stride(0) == d + 8
            if not torch.equal(_rowdot(XI, VI[:, :d]).double(), XI.double() @ VI[:, :d].double().t()):
                wrong.append(("integers", nv, N))
            got = _rowdot(XF, VF[:, :d])
            X64, V64 = XF.double(), VF[:, :d].double()
            err, bound = (got.double() - X64 @ V64.t()).abs(), d * U * (X64.abs() @ V64.abs().t())
            worst = max(worst, float((err / bound).max()))
            if not bool((err <= bound).all()):
                wrong.append(("floats", nv, N, float((err / bound).max())))
            if N == 65536 + 17:
                assert torch.equal(ops.rowdot(XF, VF[:, :d].contiguous()), got)   # the wrapper, contiguous V
    print(f"\nGRAMSTAT rowdot d={d}: worst err / bound = {worst:.4f}")
    assert not wrong, wrong


# ---- 5. transform_bwd_prep

def _prep_inputs(din, D, n):
    """the operands and the fp64 restatement of test_transform_bwd_prep_matches_torch_formula (tests/test_gpu_training.py)"""
    from bridged_gnn_amd import ops
    g = _gen(din + D)
    ld = ops.pad4(D)
    x = torch.randn(n, din, device=DEV, generator=g)
    G1 = torch.zeros(n, ld, device=DEV); G2 = torch.zeros(n, ld, device=DEV)
    G1[:, :D] = torch.randn(n, D, device=DEV, generator=g); G2[:, :D] = torch.randn(n, D, device=DEV, generator=g)
    m = torch.rand(n, device=DEV, generator=g) < 0.4
    gx = torch.randn(2, din, device=DEV, generator=g) * 0.2
    gconst = torch.randn(2, device=DEV, generator=g) * 0.3
    wd = torch.zeros(2, 2 * D, device=DEV)
    wd[0, :D] = torch.randn(D, device=DEV, generator=g); wd[1, D:] = torch.randn(D, device=DEV, generator=g)
    counts = torch.tensor([float(m.sum()), float((~m).sum())], dtype=torch.float64, device=DEV)
    gam = torch.tanh(x.double() @ gx.double().t() + gconst.double())
    zero = gam.new_zeros(())
    want_side = torch.stack((torch.where(m, gam[:, 0], zero), torch.where(m, zero, gam[:, 1]),
                             torch.ones_like(gam[:, 0]), torch.zeros_like(gam[:, 0])), dim=1)
    cat = torch.cat((G1[:, :D], G2[:, :D]), dim=1).double()
    dc = cat @ wd.double().t()
    dpre = torch.where(torch.stack((m, ~m), dim=1), dc * (1 - gam * gam), zero)
    p = ops.pad4(2 * D + 3)
    want = torch.zeros(n, p, dtype=torch.float64, device=DEV)
    want[:, :2 * D], want[:, 2 * D:2 * D + 2] = cat, dpre
    want[:, 2 * D + 2] = torch.where(m, 1.0 / counts[0], -1.0 / counts[1])
    full = want.t() @ want_side                                                  # [p, 4] in fp64
    want_ex = torch.zeros_like(full)
    want_ex[:D, 0], want_ex[D:2 * D, 1], want_ex[:2 * D + 2, 2] = full[:D, 0], full[D:2 * D, 1], full[:2 * D + 2, 2]
    return dict(x=x, G1=G1, G2=G2, m=m, m8=m.to(torch.uint8), gx=gx, gconst=gconst, wd=wd, counts=counts, p=p, cat=cat,
                want=want, want_side=want_side, want_ex=want_ex, atol_gall=1e-5 * float(dc.abs().max()),
                atol_ex=2e-5 * float(full.abs().max()))


def _assert_gall(c, D, Gall):
    assert Gall.shape == c["want"].shape
    assert torch.equal(Gall[:, :2 * D].double(), c["cat"])
    assert torch.allclose(Gall.double(), c["want"], rtol=1e-5, atol=c["atol_gall"])


def _assert_ex(c, ex):
    assert torch.allclose(ex.double(), c["want_ex"], rtol=1e-4, atol=c["atol_ex"]), float((ex.double() - c["want_ex"]).abs().max())


@pytest.mark.parametrize("din,D,n", [(128, 128, 70001),     # EX, four column chunks per lane, grid cap 2048
                                     (128, 2, 263003),      # EX, one chunk, p = 8: grid cap 8192
                                     (256, 64, 70001),      # x wider than the registers that hold a row of it
                                     (36, 130, 263003)])    # D > 128: no ex, the side table is written
def test_transform_bwd_prep_with_four_rows_in_flight(din, D, n):
    """n > 3 x (grid x 8) rows: every lane group runs the loop that keeps four rows in flight (then the one-row remainder).
    The kernel is row-local, so the rows of Gall (and side) must equal, bit for bit, those of separate calls on 4096-row
    slices with the same `counts` -- those give every lane group one row, i.e. the remainder loop alone."""
    from bridged_gnn_amd import ops
    c = _prep_inputs(din, D, n)
    ex_route = D <= 128
    assert n > 3 * (2048 if ex_route and c["p"] > 16 else 8192) * 8              # bgnn_gram.hip prep_blocks: blocks of 8 rows, capped

    def call(lo, hi):
        return ops.transform_bwd_prep(c["x"][lo:hi], c["G1"][lo:hi], c["G2"][lo:hi], D, c["m8"][lo:hi], c["gx"], c["gconst"], c["wd"],
                                      c["counts"], want_ex=ex_route)
    Gall, second = call(0, n)
    _assert_gall(c, D, Gall)
    Gall2, second2 = call(0, n)
    assert torch.equal(Gall2, Gall) and torch.equal(second2, second), "two calls differ"
    if ex_route:
        _assert_ex(c, second)
    else:
        assert torch.allclose(second.double(), c["want_side"], rtol=1e-5, atol=2e-6)
    for lo in (0, (n // 2) & ~7 | 3, n - 4096):
        g_small, s_small = call(lo, lo + 4096)
        assert torch.equal(Gall[lo:lo + 4096], g_small), f"Gall rows {lo}..{lo + 4096} differ from a 4096-row call"
        if not ex_route:
            assert torch.equal(second[lo:lo + 4096], s_small), f"side rows {lo}..{lo + 4096} differ from a 4096-row call"


def test_transform_bwd_prep_with_four_rows_in_flight_into_a_pair_buffer():
    """as _TransformPairFn.backward calls it: out = (the second half of a [N, 2p] buffer, None), want_ex"""
    from bridged_gnn_amd import ops
    din, D, n = 64, 3, 263003
    c = _prep_inputs(din, D, n)
    p = c["p"]
    wide = torch.full((n, 2 * p), float("nan"), device=DEV)
    Gall, ex = ops.transform_bwd_prep(c["x"], c["G1"], c["G2"], D, c["m8"], c["gx"], c["gconst"], c["wd"], c["counts"],
                                      out=(wide[:, p:], None), want_ex=True)
    assert Gall.data_ptr() == wide[:, p:].data_ptr() and bool(torch.isnan(wide[:, :p]).all()), "the other conv's half was written"
    _assert_gall(c, D, wide[:, p:])
    _assert_ex(c, ex)
    alone, ex_alone = ops.transform_bwd_prep(c["x"], c["G1"], c["G2"], D, c["m8"], c["gx"], c["gconst"], c["wd"], c["counts"], want_ex=True)
    assert torch.equal(alone, wide[:, p:]) and torch.equal(ex_alone, ex)
    lo = n - 4096
    small = ops.transform_bwd_prep(c["x"][lo:], c["G1"][lo:], c["G2"][lo:], D, c["m8"][lo:], c["gx"], c["gconst"], c["wd"], c["counts"],
                                   want_ex=True)[0]
    assert torch.equal(wide[lo:, p:], small)
