"""ORACLE -- TEST INFRASTRUCTURE ONLY.  CPU torch (fp32/fp64, autograd) restatement of AdaptedConv /
KTGNN_no_complement in the reference's op order (index_select / elementwise / index_add_), used as the
checker for GRADIENTS (tests/test_gpu_training.py).  Its forward is pinned against oracle_np / the golden
vectors in tests/test_oracle_torch.py.  Citations relative to /root/reference/Bridged-GNN/."""
import torch
import torch.nn.functional as F


def segment_softmax(src, index, n):
    """torch_geometric.utils.softmax (call site models/KTGNN.py:299)"""
    m = torch.full((n,), float("-inf"), dtype=src.dtype).scatter_reduce(0, index, src, reduce="amax", include_self=True)
    e = (src - m[index]).exp()
    s = torch.zeros(n, dtype=src.dtype).index_add_(0, index, e)
    return e / (s[index] + 1e-16)


def _leaky(z, slope, flip):
    """F.leaky_relu; `flip` (bool, z's shape): those elements take the OTHER slope (a kink flip, see ktgnn_train)"""
    a = F.leaky_relu(z, slope)
    return a if flip is None else torch.where(flip, torch.where(z > 0, z * slope, z), a)


def adaptedconv(x, mask, e1, e2, p, slope=0.1, flip=None, record=None):
    """models/KTGNN.py:263-315.  p: dict of tensors (may require grad); with "lin_r.weight" the root term of :309-310.
    flip: (mask over edge_index1's, mask over edge_index2's leaky-ReLU inputs) taking the other slope; record: list that gets the
    (detached) pair of leaky-ReLU inputs appended."""
    n = x.shape[0]
    diff = (x[mask].mean(0, keepdim=True) - x[~mask].mean(0, keepdim=True)).expand(x.shape)
    cat = torch.cat((x, diff), -1)
    s2t = torch.tanh(cat @ p["a_g_s2t.weight"].t()) * diff
    t2s = torch.tanh(cat @ p["a_g_t2s.weight"].t()) * diff
    h_s2t = F.linear(x - s2t * mask.unsqueeze(-1), p["lin_t.weight"], p.get("lin_t.bias"))
    h_t2s = F.linear(x + t2s * (~mask).unsqueeze(-1), p["lin_s.weight"], p.get("lin_s.bias"))
    z1, z2 = h_t2s[e1[0]] + h_t2s[e1[1]], h_s2t[e2[0]] + h_s2t[e2[1]]
    if record is not None:
        record.append((z1.detach(), z2.detach()))
    fl = flip if flip is not None else (None, None)
    a1 = _leaky(z1, slope, fl[0]) @ p["a_f_t2s.weight"].reshape(-1)
    a2 = _leaky(z2, slope, fl[1]) @ p["a_f_s2t.weight"].reshape(-1)
    alpha = segment_softmax(torch.cat((a1, a2)), torch.cat((e1[1], e2[1])), n)
    out = torch.zeros(n, h_s2t.shape[1], dtype=x.dtype)
    out = out.index_add(0, e1[1], h_t2s[e1[0]] * alpha[: e1.shape[1], None])
    out = out.index_add(0, e2[1], h_s2t[e2[0]] * alpha[e1.shape[1]:, None])
    if "lin_r.weight" in p:
        out = out + F.linear(x, p["lin_r.weight"])
    return out


def batchnorm_train(x, p, bufs, prefix, momentum=0.1, eps=1e-5):
    """BatchNorm1d in train mode (KTGNN.py:427, :367): normalise with the batch mean and biased variance; the running buffers
    in `bufs` move in place to (1 - momentum) old + momentum (batch mean | unbiased batch variance)."""
    n = x.shape[0]
    mu = x.mean(0)
    var = ((x - mu) ** 2).mean(0)
    with torch.no_grad():
        rm, rv = bufs[prefix + "running_mean"], bufs[prefix + "running_var"]
        rm.mul_(1 - momentum).add_(mu.detach().to(rm.dtype) * momentum)
        rv.mul_(1 - momentum).add_(var.detach().to(rv.dtype) * (n / (n - 1)) * momentum)
        bufs[prefix + "num_batches_tracked"].add_(1)
    return (x - mu) / torch.sqrt(var + eps) * p[prefix + "weight"] + p[prefix + "bias"]


def ktgnn_train(x, mask, e1, e2, p, bufs, slope=0.1, flips=None, record=None):
    """KTGNN_no_complement.forward in train mode (KTGNN.py:400-435) with use_bn=True and dropout 0 -> the three log-prob
    tensors (base, target, transformed target).  p: state_dict-named parameters (may require grad); bufs: the BatchNorm
    buffers, updated in place.  The layer count and root_weight follow from the keys.  flips: {conv call index: adaptedconv
    `flip`}, record: list for the leaky-ReLU inputs of every conv call, in call order (hidden convs, clf_base, clf_target(h),
    clf_target(clf_transformer(h)))."""
    calls = []

    def conv(name, h):
        i = len(calls)
        calls.append(name)
        return adaptedconv(h, mask, e1, e2, {k[len(name) + 1:]: v for k, v in p.items() if k.startswith(name + ".")}, slope,
                           flip=(flips or {}).get(i), record=record)
    h = x
    n_convs = len({k.split(".")[1] for k in p if k.startswith("convs.")})
    for i in range(n_convs):
        h = torch.relu(batchnorm_train(conv(f"convs.{i}", h), p, bufs, f"bns.{i}."))
    t = F.linear(h, p["clf_transformer.0.weight"], p["clf_transformer.0.bias"])
    t = torch.relu(batchnorm_train(t, p, bufs, "clf_transformer.1."))
    t = F.linear(t, p["clf_transformer.3.weight"], p["clf_transformer.3.bias"])
    return (torch.log_softmax(conv("clf_base", h), 1), torch.log_softmax(conv("clf_target", h), 1),
            torch.log_softmax(conv("clf_target", t), 1))


def graph_partition(edge_index, mask):
    n = mask.shape[0]
    ei = edge_index[:, edge_index[0] != edge_index[1]]
    loop = torch.arange(n)
    ei = torch.cat([ei, torch.stack([loop, loop])], 1)
    m1 = mask[ei[1]]
    return ei[:, m1], ei[:, ~m1]


def train_loss_terms(logp_s, logp_t, logp_that, y, train_mask, central_mask):
    """the four terms (l_s, l_t1, l_t2, l_kl) of main_graph_knowledge_transfer.py:44-52"""
    tm_t = train_mask & ~central_mask
    l_s = F.nll_loss(logp_s[train_mask], y[train_mask])
    l_t1 = F.nll_loss(logp_t[tm_t], y[tm_t])
    l_t2 = F.nll_loss(logp_that[tm_t], y[tm_t])
    l_kl = F.kl_div(logp_that, logp_t, log_target=True, reduction="batchmean")
    return l_s, l_t1, l_t2, l_kl


def train_loss(logp_s, logp_t, logp_that, y, train_mask, central_mask, Lambda=1.0):
    """main_graph_knowledge_transfer.py:44-54"""
    l_s, l_t1, l_t2, l_kl = train_loss_terms(logp_s, logp_t, logp_that, y, train_mask, central_mask)
    return (l_s * 2.0 + l_t1 + l_t2) / 4.0 + l_kl * Lambda
