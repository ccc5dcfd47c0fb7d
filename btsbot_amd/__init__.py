"""btsbot_amd -- MI355X-native implementation of BTSbot's classifier forward/backward path.

Mirrors the public surface of the reference package for this path
(/root/reference/btsbot/__init__.py:9-46): the model classes of ``architectures`` and
``load_HF_model`` / ``download_HF_model``.  Importing this package never touches a GPU; the HIP
library is loaded the first time a model is constructed and there is no CPU fallback.
"""
__version__ = "0.1.0"

import os as _os

# ScoreStream (pipeline.py) overlaps consecutive batches on two or more HIP streams; the runtime multiplexes streams
# onto GPU_MAX_HW_QUEUES hardware queues (default 4, the null stream included), and two streams that share a queue
# run one after the other.  Measured, 2 streams: 0.358 ms per batch at 4 queues, 0.341 at 8.  Read by the HIP runtime
# when it initialises (the first device call), so it only takes effect if that has not happened yet; an explicit
# setting of the user's wins.
_os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

from . import architectures
from . import from_HF
from . import to_HF
from . import data
from . import val
from . import alert_utils
from . import splits
from .architectures import (
    MaxViT,
    ConvNeXt,
    mm_MaxViT,
    mm_ConvNeXt,
    mm_cnn,
    um_cnn,
    um_nn,
    frozen_fusion,
)
from .from_HF import download_HF_model, load_HF_model
from .synthetic import METADATA_COLS, synthetic_batch
from .pipeline import ScoreStream
from .alert_utils import CUSTOM_COLS, alert_features, decode_stamps_device, make_metadata, make_triplets
from .val import REFERENCE_POLICIES, policy_eval, policy_performance
from . import diagnostics
from .diagnostics import alert_histograms, diagnostic_data, diagnostic_fig, draw_diagnostic_fig, roc_points
from .triggers import TriggerState
from .features import FeatureState
from . import neighbors
from .neighbors import (EmbeddingIndex, embedding_neighbors, knn_graph, neighbor_ranks, neighbor_vote, radius_graph,
                        radius_neighbors)
from . import ivf
from .ivf import IvfIndex, KMeansFit, kmeans
from . import mapindex
from .mapindex import MapIndex
from . import clusters
from .clusters import dbscan, graph_components
from . import quality
from .quality import continuity, map_quality, trustworthiness
from . import graph
from .graph import KnnGraph
from . import novelty
from .novelty import NoveltyModel, kth_neighbor_distance, local_outlier_factor
# (the function takes the package attribute ``hdbscan``; the module is ``from btsbot_amd.hdbscan import ...``)
from .hdbscan import ClusterModel, ClusterTree, MutualReachabilityMST, hdbscan, mutual_reachability_mst
from . import attribution
from .attribution import saliency
from . import layout
from .layout import (EmbeddingMap, FuzzyGraph, embedding_layout, find_ab_params, fuzzy_graph, layout_transform,
                     optimize_layout, query_memberships)
from .splits import (SOURCE_SETS, SPLIT_NAMES, create_subset, cut_set_and_assign_splits, cuts_suffix, label_set,
                     merge_sets_across_split, split_labels, subsample_data, subset_mask)

__all__ = [
    "__version__", "architectures", "from_HF", "to_HF", "data", "val", "alert_utils",
    "MaxViT", "ConvNeXt", "mm_MaxViT", "mm_ConvNeXt", "mm_cnn", "um_cnn", "um_nn", "frozen_fusion",
    "download_HF_model", "load_HF_model", "METADATA_COLS", "synthetic_batch", "ScoreStream",
    "CUSTOM_COLS", "alert_features", "make_metadata", "make_triplets", "decode_stamps_device",
    "REFERENCE_POLICIES", "policy_eval", "policy_performance", "triggers", "TriggerState",
    "diagnostics", "alert_histograms", "roc_points", "diagnostic_data", "diagnostic_fig", "draw_diagnostic_fig",
    "features", "FeatureState",
    "neighbors", "EmbeddingIndex", "embedding_neighbors", "knn_graph", "neighbor_vote",
    "radius_neighbors", "radius_graph", "neighbor_ranks", "quality", "trustworthiness", "continuity", "map_quality",
    "clusters", "graph_components", "dbscan", "mapindex", "MapIndex",
    "graph", "KnnGraph",
    "ivf", "IvfIndex", "KMeansFit", "kmeans",
    "novelty", "NoveltyModel", "local_outlier_factor", "kth_neighbor_distance",
    "hdbscan", "mutual_reachability_mst", "MutualReachabilityMST", "ClusterTree", "ClusterModel",
    "attribution", "saliency",
    "layout", "FuzzyGraph", "fuzzy_graph", "optimize_layout", "embedding_layout", "find_ab_params",
    "EmbeddingMap", "layout_transform", "query_memberships",
    "splits", "SPLIT_NAMES", "SOURCE_SETS", "label_set", "split_labels", "subset_mask", "cuts_suffix",
    "cut_set_and_assign_splits", "merge_sets_across_split", "create_subset", "subsample_data",
]
