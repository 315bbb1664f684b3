"""CPU: the fused Adam's C entry is declared, exported and bound; the `--graphed` switch parses; the host-side tables of a captured
epoch (learning rates, dropout seeds) are the numbers an eager run produces."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from bridged_gnn_amd import transfer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RUN_SH_STEP2 = (
    "--num_layer 2 --hidden_dim 128 --path_data ../data_bridged_graph/twitter_unrelational_bridged_graph.dat --to_undirected",
    "--num_layer 2 --hidden_dim 64 --path_data ../data_bridged_graph/office_amazon2dslr_bridged_graph.dat --to_undirected",
    "--num_layer 2 --hidden_dim 128 --path_data ../data_bridged_graph/office_amazon2webcam_bridged_graph.dat --to_undirected",
    "--num_epoch 300 --num_layer 2 --hidden_dim 64 --path_data ../data_bridged_graph/fb_hamilton2caltech_bridged_graph.dat --to_undirected --no_dtc",
    "--num_epoch 200 --num_layer 2 --hidden_dim 64 --path_data ../data_bridged_graph/fb_howard2simmons_bridged_graph.dat",
)


def test_adam_entry_is_declared_exported_and_bound():
    from bridged_gnn_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bgnn.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.SO_PATH)
    for name in ("bgnn_adam_step_f32", "bgnn_adam_chunk_elems"):
        assert re.search(r"\b" + name + r"\s*\(", txt), f"{name} is not declared in include/bgnn.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES
    assert "main_graph_knowledge_transfer.py:205, :67, :353, :274" in open(os.path.join(ROOT, "include", "bgnn.h")).read()
    assert "bgnn_optim.hip" in _lib._HASHED_SOURCES
    assert "bgnn_optim.hip" in open(os.path.join(ROOT, "bridged_gnn_amd", "csrc", "Makefile")).read()
    assert _lib.ABI_VERSION == 116 and _lib.lib().bgnn_version() == 116
    chunk = _lib.lib().bgnn_adam_chunk_elems()
    assert chunk > 0 and chunk % 4 == 0


def test_fused_adam_refuses_host_tensors():
    from bridged_gnn_amd.optim import FusedAdam
    with pytest.raises(RuntimeError, match="no CPU"):
        FusedAdam([torch.zeros(4, requires_grad=True)], lr=1e-3)
    with pytest.raises(ValueError):
        FusedAdam([], lr=1e-3)


@pytest.mark.parametrize("line", RUN_SH_STEP2)
def test_graphed_flag_is_off_in_the_references_command_lines(line):
    a = transfer.build_parser().parse_args(line.split())
    assert a.graphed is False
    b = transfer.build_parser().parse_args(line.split() + ["--graphed"])
    assert b.graphed is True
    for k, v in vars(a).items():
        assert k == "graphed" or getattr(b, k) == v


def test_graphed_keyword_is_additive_and_off_by_default():
    for fn in (transfer.train_gnn, transfer.train_gnn_noDTC):
        sig = inspect.signature(fn).parameters
        assert list(sig)[-1] == "graphed" and sig["graphed"].default is False


@pytest.mark.parametrize("lr,step_size,gamma,epochs", [(1e-3, 100, 0.1, 300), (1e-3, 3, 0.1, 8), (5e-3, 7, 0.3, 50)])
def test_lr_table_is_the_schedulers_own_sequence(lr, step_size, gamma, epochs):
    from torch.optim.lr_scheduler import StepLR
    from bridged_gnn_amd.optim import lr_table
    tab = lr_table(lr, epochs, step_size, gamma)
    assert tab.dtype == torch.float64 and tab.shape == (epochs,)
    opt = torch.optim.Adam([torch.zeros(3, requires_grad=True)], lr=lr, weight_decay=5e-3)
    sched = StepLR(opt, step_size=step_size, gamma=gamma)
    want = []
    for _ in range(epochs):
        want.append(sched.get_last_lr()[0])             # the rate this epoch's optimizer.step() uses
        opt.step()
        sched.step()
    assert tab.tolist() == want                         # bit for bit: both are Python floats (fp64)
    if epochs == 300:                                    # the reference's schedule really decays, and not as lr * gamma ** k everywhere
        assert tab[0] == 1e-3 and tab[99] == 1e-3 and tab[100] < 1.1e-4 and tab[299] < 1.1e-5
    const = lr_table(lr, epochs)
    assert const.tolist() == [lr] * epochs and lr_table(lr, 0).tolist() == [lr]


@pytest.mark.parametrize("layers", [1, 2])
def test_pre_drawn_seeds_are_the_eager_loops_draws(layers):
    from bridged_gnn_amd.optim import draw_dropout_seeds
    E = 7
    torch.manual_seed(11)
    eager = []
    for _ in range(E):                                   # an eager epoch: one host draw per dropout layer (ktgnn._BnReluDropFn, sage.SAGEConv.run)
        eager.append([int(torch.empty((), dtype=torch.int64).random_().item()) for _ in range(layers)])
    after = torch.get_rng_state()
    torch.manual_seed(11)
    tab = draw_dropout_seeds(E, layers)
    assert tab.dtype == torch.int64 and tab.tolist() == eager
    assert torch.equal(torch.get_rng_state(), after)
    assert len(set(sum(eager, []))) == E * layers        # (the draws differ from one another: the comparison says something)
    before = torch.get_rng_state()
    assert draw_dropout_seeds(0, layers).shape == (0, layers) and draw_dropout_seeds(E, 0).shape == (E, 0)
    assert torch.equal(torch.get_rng_state(), before)


def test_seed_feed_hands_out_one_word_per_layer_without_drawing():
    from bridged_gnn_amd import ktgnn
    words = torch.arange(2, dtype=torch.int64)
    feed = ktgnn.DropoutSeedFeed(words)
    before = torch.get_rng_state()
    ktgnn._DROPOUT_STEP[0] = feed
    try:
        s0, w0 = ktgnn.dropout_seed(0.5)
        s1, w1 = ktgnn.dropout_seed(0.0)                 # a layer without dropout takes no word
        s2, w2 = ktgnn.dropout_seed(0.5, step_word=False)
        assert (s0, s1, s2) == (0, 0, 0) and w1 is None
        assert w0.data_ptr() == words.data_ptr() and w2.data_ptr() == words.data_ptr() + 8 and feed.taken == 2
        with pytest.raises(RuntimeError, match="more dropout layers"):
            ktgnn.dropout_seed(0.5)
        feed.rewind()
        assert feed.taken == 0
    finally:
        ktgnn._DROPOUT_STEP[0] = None
    assert torch.equal(torch.get_rng_state(), before)
    s, w = ktgnn.dropout_seed(0.5)                       # eager: a host draw, no device word
    assert w is None and s > 0 and not torch.equal(torch.get_rng_state(), before)
