"""TEST INFRASTRUCTURE.  The cases of the training-gradient fixtures (tests/golden/grads_*.npz, written by
`oracle/gen_golden.py --only grads`): their configuration, their inputs and initial weights, and the compact form in which the
reference's fp64 results are stored.  The reference tree is not needed.

Inputs and weights are regenerated here from seeds rather than stored (the office case reads the shipped office graph from
tests/golden); the fixture keeps a sha256 of each, so a change of the generators fails loudly in `load` instead of silently testing
other inputs.  Tensors of more than FULL_MAX elements are stored as a `summary`: a strided grid of rows x columns (first, spread,
last four), every row sum and column sum (fp64 over ALL elements), the max |value| and the sum of squares.  The fp64 torch oracle
(`oracle_torch.ktgnn_train`) is pinned to these summaries at 1e-10 (tests/test_oracle_torch.py), and the GPU test compares the
HIP step with that oracle on full tensors (tests/test_gpu_grads_reference.py)."""
import hashlib
import os
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")

# case -> (graph, num_features, hidden, num_classes, layer_num, root_weight, seed)
CASES = {
    "office64": ("office", 256, 64, 31, 2, False, 20),
    "office128": ("office", 256, 128, 31, 2, False, 21),
    "heads3": ("m", 48, 64, 3, 2, False, 22),
    "odd4": ("s", 37, 64, 4, 2, False, 23),
    "c3": ("s", 300, 128, 2, 2, False, 24),
    "wide5": ("s", 64, 256, 5, 2, False, 25),
    "l3": ("s", 32, 64, 3, 3, False, 26),
    "root": ("s", 48, 64, 3, 2, True, 27),
}
GRAPHS = {"s": (700, 6000, 31, 300), "m": (4200, 36000, 32, 48)}      # tag -> (nodes, random edges, seed, feature columns)
FULL_MAX = 1024
_FILES = {}


def fixture_file(case):
    return "grads_office_a2d.npz" if CASES[case][0] == "office" else "grads_small.npz"


def multigraph(n, e, seed):
    """Seeded directed multigraph -> (edge_index int64 [2, E], central_mask bool [n]).  Uniform random edges plus: self loops and
    duplicate edges; 8 isolated nodes (the last 8 rows); 10 nodes whose in-edges all come from the other domain; rows 0..31 in the
    target domain; one destination with 320 in-edges and one source with 320 out-edges (both above ops.HUB_THRESHOLD = 128, so
    both hub tables of the pull backward are built)."""
    rng = np.random.default_rng(seed)
    mask = rng.random(n) < 0.45
    mask[:32] = False
    iso, cross_only = np.arange(n - 8, n), np.arange(40, 50)
    hub_in, hub_out = n // 2, n // 2 + 1
    src, dst = rng.integers(0, n, e), rng.integers(0, n, e)
    src = np.concatenate([src, rng.integers(0, n, 320), np.full(320, hub_out)])
    dst = np.concatenate([dst, np.full(320, hub_in), rng.integers(0, n, 320)])
    loops = rng.integers(0, n, 24)
    src, dst = np.concatenate([src, loops]), np.concatenate([dst, loops])
    dup = rng.integers(0, src.size, e // 20)
    src, dst = np.concatenate([src, src[dup]]), np.concatenate([dst, dst[dup]])
    keep = ~(np.isin(src, iso) | np.isin(dst, iso)) & ~(np.isin(dst, cross_only) & (mask[src] == mask[dst]))
    src, dst = src[keep], dst[keep]
    other = [np.flatnonzero(mask != mask[c])[:3] for c in cross_only]                  # at least three cross in-edges each
    src = np.concatenate([src] + other)
    dst = np.concatenate([dst] + [np.full(3, c) for c in cross_only])
    perm = rng.permutation(src.size)
    return np.stack([src[perm], dst[perm]]).astype(np.int64), mask


def _npz(name):
    if name not in _FILES:
        _FILES[name] = dict(np.load(os.path.join(GOLDEN, name)))
    return _FILES[name]


def graph(tag):
    """-> (x float32 [N, F], edge_index int64 [2, E], central_mask).  'office': the shipped office A->D graph, undirected (as
    ktgnn_office.npz); 's' / 'm': `multigraph` with seeded features of fp16-exact values and a domain shift the gates can see."""
    if tag == "office":
        g = _npz("office_a2d_graph.npz")
        return g["x"], _npz("partition_office.npz")["ei_undirected"].astype(np.int64), g["central_mask"]
    n, e, seed, cols = GRAPHS[tag]
    ei, cm = multigraph(n, e, seed)
    x = np.random.default_rng(seed + 100).standard_normal((n, cols)) + 0.5 * cm[:, None]
    return x.astype(np.float16).astype(np.float32), ei, cm


def labels(case, n):
    """-> (y int64 [n], train_mask bool [n]); the office cases use the shipped labels and split"""
    gname, _, _, C, _, _, seed = CASES[case]
    if gname == "office":
        g = _npz("office_a2d_graph.npz")
        return g["y"].astype(np.int64), g["train_mask"]
    r = np.random.default_rng(seed)
    return r.integers(0, C, n), r.random(n) < 0.5


def init_state(case, template):
    """initial state_dict of the case as float32 arrays, from `template` (name -> array-like with .shape; any KTGNN_no_complement
    state_dict of the case's configuration).  Every entry has its own generator (seed, crc32 of the name): order-independent.
    Linear weight / bias U(-1/sqrt(fan_in), +); BatchNorm weight U(0.5, 1.5), bias and running_mean U(-0.1, 0.1), running_var
    U(0.5, 1.5), num_batches_tracked 0."""
    seed = CASES[case][6]
    bn = {k[: -len("running_mean")] for k in template if k.endswith("running_mean")}
    out = {}
    for k in sorted(template):
        shape = tuple(template[k].shape)
        if k.endswith("num_batches_tracked"):
            out[k] = np.zeros(shape, np.int64)
            continue
        rng = np.random.default_rng([seed, zlib.crc32(k.encode())])
        pre, leaf = k.rsplit(".", 1)
        pre += "."
        if pre in bn:
            lo, hi = {"weight": (0.5, 1.5), "running_var": (0.5, 1.5)}.get(leaf, (-0.1, 0.1))
        else:
            b = 1.0 / np.sqrt(template[pre + "weight"].shape[-1])
            lo, hi = -b, b
        out[k] = rng.uniform(lo, hi, shape).astype(np.float32)
    return out


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes())
    return h.hexdigest()


def spread(n, k=12):
    return np.unique(np.concatenate([np.linspace(0, n - 1, k).round().astype(np.int64), np.arange(max(n - 4, 0), n)]))


def summary(a):
    """the stored form of a result tensor (fp64): in full up to FULL_MAX elements, else grid / row sums / column sums / amax /
    sum of squares (module docstring)"""
    a = np.asarray(a, np.float64)
    if a.size <= FULL_MAX:
        return {"full": a}
    m = a.reshape(a.shape[0], -1)
    return {"grid": m[np.ix_(spread(m.shape[0]), spread(m.shape[1]))], "rowsum": np.add.reduceat(m.sum(1), _blocks(m.shape[0])),
            "colsum": m.sum(0), "amax": np.float64(np.abs(m).max()), "sumsq": np.float64((m * m).sum())}


def _blocks(rows):
    """starts of the row blocks whose sums are stored: single rows up to 256 rows, then ceil(rows / 256) rows per block"""
    return np.arange(0, rows, -(-rows // 256))


def compare(got, ref, tol, scale=None):
    """-> list of (part, error / allowed) for `got` (full tensor) against a stored summary `ref`: elements within tol * scale
    (default: the tensor's max |value|), sums of n elements within tol * scale * sqrt(n), amax within tol * scale, sum of squares
    within 2 tol * scale * sum|value|.  Every ratio must be <= 1."""
    s = summary(got)
    amax = float(np.abs(ref["full"]).max()) if "full" in ref else float(ref["amax"])
    scale = amax if scale is None else scale
    scale = max(scale, 1e-300)
    if "full" in ref:
        return [("full", float(np.abs(s["full"] - ref["full"]).max()) / (tol * scale))]
    m = np.asarray(got, np.float64)
    m = m.reshape(m.shape[0], -1)
    return [("grid", float(np.abs(s["grid"] - ref["grid"]).max()) / (tol * scale)),
            ("rowsum", float(np.abs(s["rowsum"] - ref["rowsum"]).max()) / (tol * scale * np.sqrt(m.shape[1] * -(-m.shape[0] // 256)))),
            ("colsum", float(np.abs(s["colsum"] - ref["colsum"]).max()) / (tol * scale * np.sqrt(m.shape[0]))),
            ("amax", abs(float(s["amax"]) - amax) / (tol * scale)),
            ("sumsq", abs(float(s["sumsq"]) - float(ref["sumsq"])) / (2 * tol * scale * float(np.abs(m).sum())))]


def _unpack(f, prefix):
    names = {}
    for k, v in f.items():
        if k.startswith(prefix):
            name, part = k[len(prefix):].rsplit(":", 1)
            names.setdefault(name, {})[part] = v
    return names


def pack(prefix, name, s):
    return {f"{prefix}{name}:{part}": v for part, v in s.items()}


def load(case, template=None):
    """-> dict: feat, hidden, C, layers, root, x [N, feat] float32, edge_index int64, central_mask, y, train_mask, sd (initial
    state_dict, needs `template` -- else taken from the reference shapes stored in the fixture), and the reference's fp64 step:
    loss [total, l_s, l_t1, l_t2, l_kl], grad (name -> summary), gmax (largest |gradient| of the model), dx / logp_base /
    logp_target / logp_target_hat (summaries), bn (BatchNorm buffers after the forward, full), kinks_leaky_relu / kinks_relu
    [calls, 2] (inputs within 1e-6 / 1e-7 of their tensor's max of zero)."""
    gname, feat, hidden, C, layers, root, _ = CASES[case]
    f = _npz(fixture_file(case))
    p = case + "."
    x, ei, cm = graph(gname)
    x = np.ascontiguousarray(x[:, :feat])
    y, tm = labels(case, x.shape[0])
    assert str(f[p + "data_sha"]) == sha(x, ei, cm, y, tm), f"{case}: regenerated inputs differ from the ones the fixture was made from"
    shapes = {k[len(p + "shape:"):]: np.empty(tuple(v)) for k, v in f.items() if k.startswith(p + "shape:")}
    sd = init_state(case, template if template is not None else shapes)
    assert str(f[p + "sd_sha"]) == sha(*(sd[k] for k in sorted(sd))), f"{case}: regenerated weights differ from the fixture's"
    out = dict(feat=feat, hidden=hidden, C=C, layers=layers, root=root, x=x, edge_index=ei, central_mask=cm, y=y, train_mask=tm,
               sd=sd, loss=f[p + "loss"], gmax=float(f[p + "gmax"]), grad=_unpack(f, p + "grad."),
               bn={k[len(p + "bn."):]: v for k, v in f.items() if k.startswith(p + "bn.")},
               kinks_leaky_relu=f[p + "kinks_leaky_relu"], kinks_relu=f[p + "kinks_relu"])
    res = _unpack(f, p + "res.")
    out.update({k: res[k] for k in ("dx", "logp_base", "logp_target", "logp_target_hat")})
    return out


def oracle_step(c, flips=None, record=None):
    """one training step of the fp64 torch oracle (oracle_torch.ktgnn_train + train_loss, CPU) on a `load`ed case -> dict of
    numpy arrays: logp_base / logp_target / logp_target_hat, loss [total, l_s, l_t1, l_t2, l_kl], grad (name -> full gradient),
    dx, bn (the BatchNorm buffers after the forward).  flips / record: see oracle_torch.ktgnn_train"""
    import torch
    from oracle import oracle_torch as OT
    mask = torch.from_numpy(c["central_mask"])
    e1, e2 = OT.graph_partition(torch.from_numpy(c["edge_index"]), mask)
    bn = {k for k in c["sd"] if k.endswith(("running_mean", "running_var", "num_batches_tracked"))}
    p = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in c["sd"].items() if k not in bn}
    bufs = {k: torch.from_numpy(c["sd"][k].copy()) for k in bn}
    bufs = {k: v.double() if v.is_floating_point() else v for k, v in bufs.items()}
    x = torch.from_numpy(c["x"]).double().requires_grad_(True)
    y, tm = torch.from_numpy(c["y"]), torch.from_numpy(c["train_mask"])
    outs = OT.ktgnn_train(x, mask, e1, e2, p, bufs, flips=flips, record=record)
    terms = OT.train_loss_terms(*outs, y, tm, mask)
    loss = OT.train_loss(*outs, y, tm, mask)
    loss.backward()
    r = {nm: o.detach().numpy() for nm, o in zip(("logp_base", "logp_target", "logp_target_hat"), outs)}
    r.update(loss=np.array([loss.item()] + [t.item() for t in terms]), grad={k: v.grad.numpy() for k, v in p.items()},
             dx=x.grad.numpy(), bn={k: v.numpy() for k, v in bufs.items()})
    return r
