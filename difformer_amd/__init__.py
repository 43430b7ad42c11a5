"""difformer_amd -- MI355X-native DIFFormer propagation layer (drop-in for the reference `difformer` module).

    from difformer_amd import DIFFormer
    model = DIFFormer(in_channels, hidden_channels, out_channels, use_graph=True, kernel='simple').cuda()
    logits = model(x, edge_index)

The arithmetic lives in lib/libdifformer_hip.so (hand-written gfx950 kernels, C ABI in
include/difformer_hip.h) and, for the attention maps, lib/libdifformer_maps.so (top-k per row,
include/difformer_maps.h) and lib/libdifformer_edges.so (at the edges of a graph, include/difformer_edges.h); k-nearest-neighbour
graphs come from lib/libdifformer_knn.so (include/difformer_knn.h) and, for a batch of graphs stored back to back (knn_graph
with batch= / n_nodes=, radius_graph), from lib/libdifformer_nbr.so (include/difformer_nbr.h), the evaluation metrics from lib/libdifformer_metrics.so
(include/difformer_metrics.h), the training losses (masked log-softmax NLL, BCE with logits) from lib/libdifformer_loss.so
(include/difformer_loss.h), the Adam update of a whole model in one launch from lib/libdifformer_adam.so
(include/difformer_adam.h), the graph read-out (global_add_pool / global_mean_pool / global_max_pool behind GraphGNN) from
lib/libdifformer_readout.so (include/difformer_readout.h), all snapshots of a spatial-temporal epoch in one launch per pass
(SnapshotBatch, DIFFormer.forward_snapshots) from lib/libdifformer_snapshots.so (include/difformer_snapshots.h).  Importing this package does not load the library; the first operator
call does, and fails loudly if it has not been built.
"""
from .attention_maps import attention_on_edges, attention_topk  # noqa: F401
from .difformer import DIFFormer, DIFFormerConv, full_attention_conv, gcn_conv  # noqa: F401
from .difformer_v2 import DIFFormer_v2, TransConv  # noqa: F401
from .dist import RowShard  # noqa: F401
from .graphs import GraphedForward, GraphedTrainStep, graphed_training  # noqa: F401
from .losses import bce_with_logits, log_softmax_nll, loss_record  # noqa: F401
from .metrics import eval_acc, eval_f1, eval_rocauc, rocauc_counts  # noqa: F401
from .neighbors import kneighbors_graph, knn_graph, radius_graph  # noqa: F401
from .optim import Adam  # noqa: F401
from .readout import GraphGNN, global_add_pool, global_max_pool, global_mean_pool  # noqa: F401
from .snapshots import SnapshotBatch  # noqa: F401

__all__ = ["DIFFormer", "DIFFormerConv", "full_attention_conv", "gcn_conv", "DIFFormer_v2", "TransConv", "RowShard",
           "GraphedForward", "GraphedTrainStep", "graphed_training", "attention_topk", "attention_on_edges", "knn_graph",
           "kneighbors_graph", "radius_graph", "eval_rocauc", "eval_acc", "eval_f1", "rocauc_counts", "log_softmax_nll",
           "bce_with_logits", "loss_record", "Adam", "global_add_pool", "global_mean_pool", "global_max_pool", "GraphGNN",
           "SnapshotBatch"]
__version__ = "0.1.0"
