"""MI355X-native (gfx950) implementation of Bridged-GNN's sparse message-passing hot path.

Half A: bridged-graph kNN construction (`bridge.py`) -- reference `main_bridged_graph.py:33-120`.
Half B: KT-GNN `AdaptedConv` aggregation (`ktgnn.py`) -- reference `models/KTGNN.py:218-435`.
Compute goes through the C-ABI library `csrc/libbgnn_hip.so` (declared in `include/bgnn.h`);
there is no CPU fallback: ops raise if the library or a GPU tensor is missing.
"""
from .data import Data, load_bridged_graph, save_bridged_graph  # noqa: F401

__version__ = "0.1.0"


def __getattr__(name):
    # the GCN baseline's classes, imported on first use (they pull in the HIP library's binding)
    if name in ("GCNNet", "GCNConv"):
        from . import gcn
        return getattr(gcn, name)
    if name in ("GAT", "GATConv"):                     # the GAT baseline's, likewise
        from . import gat
        return getattr(gat, name)
    if name in ("GATv2", "GATv2Conv"):                 # the GATv2 baseline's, likewise
        from . import gatv2
        return getattr(gatv2, name)
    if name in ("APPNP", "APPNP_Net"):                 # the APPNP baseline's, likewise
        from . import appnp
        return getattr(appnp, name)
    if name in ("GCN2", "GCN2Conv", "train_gcn2_noDTC"):   # the GCNII baseline's, likewise
        from . import gcn2
        return getattr(gcn2, name)
    if name in ("DeeperGCN", "GENConv", "DeepGCNLayer", "train_deepergcn_noDTC"):   # the DeeperGCN baseline's, likewise
        from . import deepergcn
        return getattr(deepergcn, name)
    if name in ("GINNet", "GINConv", "train_gin_noDTC"):   # the GIN baseline's, likewise
        from . import gin
        return getattr(gin, name)
    if name in ("JKNet", "JKGraph", "JumpingKnowledge", "train_jknet_noDTC"):   # the JKNet baseline's, likewise
        from . import jknet
        return getattr(jknet, name)
    if name in ("PartitionedGCN", "GcnPartition"):     # the same model on a node partition across GPUs
        from . import dist_gcn
        return getattr(dist_gcn, name)
    if name in ("PartitionedGAT", "GatPartition"):     # the GAT baseline on a node partition, likewise
        from . import dist_gat
        return getattr(dist_gat, name)
    if name == "PartitionedGATv2":                     # the GATv2 baseline on the same partition
        from . import dist_gatv2
        return dist_gatv2.PartitionedGATv2
    if name in ("PartitionedAPPNP", "AppnpPartition"):     # the APPNP baseline on a node partition (two partitions: A and A^T)
        from . import dist_appnp
        return getattr(dist_appnp, name)
    if name == "PartitionedGCN2":                      # the GCNII baseline on the GCN partition
        from . import dist_gcn2
        return dist_gcn2.PartitionedGCN2
    if name == "PartitionedGIN":                       # the GIN baseline on the GraphSAGE partition (edges as given)
        from . import dist_gin
        return dist_gin.PartitionedGIN
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
