"""Training step of the classifier on MI355X: the hot loop of /root/reference/btsbot/train.py:481-566
(zero_grad -> forward -> BCEWithLogitsLoss(pos_weight) -> backward -> AdamW.step) plus the optimiser
and schedule set-up of train.py:242-260, without autograd, host syncs or DataParallel.

    trainer = Trainer(model, lr=1e-4, betas=(0.99, 0.99), pos_weight=w)   # model.train() already
    for images, meta, labels in batches:                                    # device tensors
        loss = trainer.step(images, meta, labels)        # returns a device scalar, no .item()
    trainer.scheduler_step()                                                # once per epoch

What is trained follows ``requires_grad`` exactly as the reference does (train.py:224-236): for
``frozen_fusion`` only ``combined_head``; otherwise everything, ConvNeXt image branch included.  With torch.distributed initialised, every rank passes its
own shard and the flat gradient arena is all-reduced once per step (parallel.py).
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Optional, Sequence

import torch

from . import _lib, parallel


def lr_schedule(lr: float, epochs: int, warmup_epochs: int) -> Sequence[float]:
    """Learning rate of epoch 0..epochs-1 under train.py:249-260's
    SequentialLR[LinearLR(0.01 -> 1 over warmup), CosineAnnealingLR(T_max=max(1, epochs-warmup),
    eta_min=0.01*lr)], stepped once per epoch -- produced by torch's own schedulers so that
    version quirks (warmup 0 leaves the LR at 0.01*lr on torch 2.10) are reproduced, not guessed."""
    import warnings
    prm = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.AdamW([prm], lr=lr)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sched = torch.optim.lr_scheduler.SequentialLR(
            opt,
            schedulers=[
                torch.optim.lr_scheduler.LinearLR(opt, start_factor=0.01, total_iters=warmup_epochs),
                torch.optim.lr_scheduler.CosineAnnealingLR(
                    opt, T_max=max(1, epochs - warmup_epochs), eta_min=lr * 0.01),
            ],
            milestones=[warmup_epochs])
        out = []
        for _ in range(epochs):
            out.append(opt.param_groups[0]["lr"])
            opt.step()
            sched.step()
    return out


_EAGER_REPACK = os.environ.get("BTSBOT_AMD_EAGER_REPACK", "1") != "0"


class Trainer:
    def __init__(self, model, lr: float = 1e-4, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, pos_weight: float = 1.0, epochs: int = 1,
                 warmup_epochs: int = 0, group=None, dropout_seed: int = 0, rccl_comm=None):
        self.model = model
        self.base_lr, self.betas, self.eps, self.wd = lr, betas, eps, weight_decay
        self.pos_weight = float(pos_weight)
        self.group = group
        self.lrs = list(lr_schedule(lr, max(1, epochs), warmup_epochs))
        self.epoch = 0
        self.t = 0                                   # AdamW step count
        comb, meta, image = model._slot_groups()
        self.need_image = any(t.requires_grad for t, *_ in image)
        self.need_meta = any(t.requires_grad for t, *_ in meta)
        # contiguous arena ranges of the trainable tensors (padding between tensors has zero grad)
        self.ranges = parallel.trainable_ranges(
            (off, numel) for t, off, numel, _s in image + meta + comb if t.requires_grad)
        # the exchange step: one all-reduce per gradient bucket, in the order btsbot_backward() finishes them
        self.exchange = parallel.GradExchange(self.ranges, model._grad_buckets(), group)
        self.exp_avg = None
        self.exp_avg_sq = None
        import torch.distributed as dist
        self.rank = dist.get_rank(group) if dist.is_available() and dist.is_initialized() else 0
        self.dropout_seed = int(dropout_seed)
        self._rng = None
        # the exchange step through the C ABI (btsbot_allreduce_grads) on a raw RCCL communicator (btsbot_amd.rccl.RcclComm)
        # instead of torch.distributed: what a host that binds only libbtsbot_hip.so does.  The replicas must then be
        # made equal by the caller (no process group to broadcast over)
        self.rccl = rccl_comm
        if rccl_comm is not None:
            self.rank = rccl_comm.rank
        # replicas start from rank 0's parameters and buffers (what DataParallel's per-step broadcast did
        # implicitly at train.py:238-240); from here on identical gradients keep them identical
        if parallel._world(group) > 1:
            parallel.broadcast_(model._arena, 0, group)
            model.mark_weights_dirty()

    @property
    def lr(self) -> float:
        return self.lrs[min(self.epoch, len(self.lrs) - 1)]

    def scheduler_step(self):
        """train.py:332 -- once per epoch."""
        self.epoch += 1

    def gradients(self, images: Optional[torch.Tensor], meta: Optional[torch.Tensor], labels: torch.Tensor,
                  global_batch: Optional[int] = None, exchange: bool = True):
        """Forward + BCE + backward (+ the exchange step when `exchange` and more than one rank) on this rank's shard,
        without the optimiser update: returns (sum_i loss_i / global_batch as a device scalar, the flat gradient arena
        -- a buffer the library reuses on the next call).  `step` is this followed by AdamW; the multi-GPU tests call it
        to compare sharded + exchanged gradients with a single-process pass over the whole batch."""
        m = self.model
        if not m.training:
            raise RuntimeError("Trainer.step: put the model in train mode first (model.train())")
        images, meta, batch, dev = m._check_inputs(images, meta)
        if labels.numel() != batch:
            raise ValueError(f"Trainer.step: {labels.numel()} labels for a batch of {batch} alerts")
        if batch < 2 and m._cfg_args["n_meta"] > 0:
            # nn.BatchNorm1d in train mode: "Expected more than 1 value per channel when training"
            raise ValueError("Trainer.step: BatchNorm1d batch statistics need more than one alert per rank")
        world = self.rccl.world if self.rccl is not None else parallel._world(self.group)
        n_global = int(global_batch) if global_batch is not None else batch * world
        if self._rng is None or self._rng.device != dev:
            # every rank draws its own dropout masks (seed + rank)
            self._rng = torch.Generator(device=dev)
            self._rng.manual_seed(self.dropout_seed + 7919 * self.rank)
        with torch.no_grad():
            masks = m._dropout_masks(batch, dev, self._rng if world > 1 else None)
            logits = m._forward_train_raw(images, meta, masks, self.need_image).reshape(-1)
            y = labels.to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
            loss = torch.zeros(1, dtype=torch.float32, device=dev)
            dl = torch.empty_like(logits)
            L = _lib.lib()
            with torch.cuda.device(dev):
                st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
                _lib.check(L.btsbot_bce_fwd_bwd(C.c_void_p(logits.data_ptr()), C.c_void_p(y.data_ptr()),
                                                self.pos_weight, batch, n_global,
                                                C.c_void_p(loss.data_ptr()), C.c_void_p(dl.data_ptr()),
                                                st), "btsbot_bce_fwd_bwd")
            grads = m._backward_raw(dl, self.need_meta, self.need_image)
            if self.rccl is not None and exchange:
                plan = self.exchange.plan
                n = len(plan)
                bk = (C.c_int32 * n)(*[b for b, _lo, _hi in plan])
                lo = (C.c_int64 * n)(*[a for _b, a, _hi in plan])
                hi = (C.c_int64 * n)(*[z for _b, _lo, z in plan])
                with torch.cuda.device(dev):
                    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
                    _lib.check(L.btsbot_allreduce_grads(m._handle.ptr, C.c_void_p(self.rccl.ptr),
                                                        C.c_void_p(grads.data_ptr()), n, bk, lo, hi, st),
                               "btsbot_allreduce_grads")
            elif world > 1 and exchange:
                # the one exchange of the step (local gradients are already scaled by 1 / n_global)
                self.exchange.exchange(grads, m._wait_grad_bucket)
            self.last_logits = logits
        return loss[0] / n_global, grads

    def step(self, images: Optional[torch.Tensor], meta: Optional[torch.Tensor],
             labels: torch.Tensor, global_batch: Optional[int] = None, exchange: bool = True) -> torch.Tensor:
        """One optimisation step on this rank's shard; returns sum_i loss_i / global_batch as a
        device scalar (the rank's contribution to the global mean loss).  (`exchange=False` leaves the all-reduce
        out: bench.py times the step both ways to report what the collective costs in wall time.)"""
        m = self.model
        loss, grads = self.gradients(images, meta, labels, global_batch, exchange)
        dev = grads.device
        with torch.no_grad():
            if self.exp_avg is None:
                self.exp_avg = torch.zeros_like(m._arena)
                self.exp_avg_sq = torch.zeros_like(m._arena)
            self.t += 1
            L = _lib.lib()
            with torch.cuda.device(dev):
                st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
                for lo, hi in self.ranges:
                    _lib.check(L.btsbot_adamw_step(
                        C.c_void_p(m._arena[lo:hi].data_ptr()), C.c_void_p(grads[lo:hi].data_ptr()),
                        C.c_void_p(self.exp_avg[lo:hi].data_ptr()),
                        C.c_void_p(self.exp_avg_sq[lo:hi].data_ptr()), hi - lo, self.lr,
                        self.betas[0], self.betas[1], self.eps, self.wd, self.t, st),
                        "btsbot_adamw_step")
            m.mark_weights_dirty()
            if _EAGER_REPACK and self.need_image:
                # the operand images of the NEXT step, queued now: the library packs them on its side stream, under the
                # next step's mask draws and stem instead of in front of its first consumer (BTSBOT_AMD_EAGER_REPACK=0: A/B).
                # The next training forward trusts this pack while the parameters' tensor versions are unchanged: code
                # that writes the arena BEHIND torch's back between two steps (a raw C-ABI kernel, `.data` edits, a
                # custom exchange) must call model.mark_weights_dirty() afterwards, or the step runs on stale images.
                if getattr(m, "_reserved_image", False):
                    with torch.cuda.device(dev):
                        m._prepare(dev, int(self.last_logits.numel()), train_only=True)   # (one logit per alert)
        return loss


def train_epoch(trainer: Trainer, dataset, epoch_metrics: bool = True):
    """train.py:481-566 for a DeviceDataset: one pass over the shuffled, augmented batches with
    ``Trainer.step`` and -- like the reference, which recomputes them on the concatenated logits
    (train.py:550-558) -- the epoch's BCE loss and accuracy, evaluated once on the device at the end
    instead of a ``.item()`` per batch.  Returns (epoch_loss, epoch_accuracy) as Python floats."""
    from .val import device_metrics
    logits, labels = [], []
    for batch in dataset:
        if len(batch) == 3:
            images, meta, y = batch
        elif dataset.images is not None:
            (images, y), meta = batch, None
        else:
            (meta, y), images = batch, None
        trainer.step(images, meta, y)
        if epoch_metrics:
            logits.append(trainer.last_logits)
            labels.append(y)
    trainer.scheduler_step()                              # train.py:332
    if not epoch_metrics or not logits:
        return float("nan"), float("nan")
    loss, acc = device_metrics(torch.cat(logits), torch.cat(labels), trainer.pos_weight)
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(trainer.group) > 1:
        both = torch.stack([loss, acc])                   # equal shards: the mean of the ranks' means
        dist.all_reduce(both, group=trainer.group)
        loss, acc = both / dist.get_world_size(trainer.group)
    return loss.item(), acc.item()


def fit(trainer: Trainer, train_set, val_images, val_metadata, val_labels, model_dir: str,
        epochs: int, patience: int = 10, val_batch_size: int = 1024, config: Optional[dict] = None,
        val_cand=None, diagnostic: bool = False, run_name: str = "diagnostic"):
    """The epoch loop of train.py:303-352 on the device: per epoch ``train_epoch`` -> ``latest_model.pth`` ->
    validation pass (val.py's loop, on the live model instead of re-instantiating it from the file) ->
    scheduler step -> ``best_model.pth`` when the validation loss improved by at least 0.5 % ->
    early stopping after ``patience`` epochs without improvement.  Checkpoints are state dicts only, like
    the reference's (no optimiser state); ``report.json`` carries ``config`` for
    to_HF.prep_config, the history and the best epoch's alert-level ``val_summary``.  ``val_cand``: the validation
    split's candidate table (a dict or DataFrame with ``objectId``, ``jd``, ``magpsf`` per validation alert, optionally
    ``junk``, ``save_time``, ``trigger_time``); with it ``val_summary`` gains the per-source ``"policy_performance"``
    (``val.policy_performance``, val.py:381-614), without it the summary is the alert-level one alone.  ``diagnostic`` (with
    ``val_cand``): rank 0 also writes ``diagnostic.json`` -- ``diagnostics.diagnostic_data`` for the best epoch, the data
    of the reference's twelve-panel figure (val.py:173-682) -- and, where matplotlib is installed, the figure itself as
    ``{run_name}.pdf``; ``report.json`` and the return value are the same with and without.  Returns the run history
    dict (train/val loss and accuracy per epoch)."""
    import json
    import os
    import numpy as np
    from .to_HF import cpu_state_dict
    from .val import run_val_tensors
    import torch.distributed as dist
    main = not (dist.is_available() and dist.is_initialized()) or dist.get_rank() == 0   # rank 0 writes the files
    if main:
        os.makedirs(model_dir, exist_ok=True)
    hist = {k: np.zeros(epochs) for k in ("train_loss", "train_accuracy", "val_loss", "val_accuracy")}
    best_raw_preds = best_val_labels = None
    since = 0
    done = 0
    for epoch in range(epochs):
        # (train_epoch also steps the LR schedule; the reference steps it after validation, with the same
        #  effect on the next epoch's learning rate)
        tl, ta = train_epoch(trainer, train_set)
        hist["train_loss"][epoch], hist["train_accuracy"][epoch] = tl, ta
        if main:
            torch.save(cpu_state_dict(trainer.model), os.path.join(model_dir, "latest_model.pth"))
        vl, va, raw, lab = run_val_tensors(trainer.model, val_images, val_metadata, val_labels,
                                           batch_size=val_batch_size, pos_weight=trainer.pos_weight)
        trainer.model.train()
        hist["val_loss"][epoch], hist["val_accuracy"][epoch] = vl, va
        done = epoch + 1
        prev_best = min([np.inf] + list(hist["val_loss"][:epoch]))
        if 1.005 * vl < prev_best:                                   # train.py:334-336
            if main:
                torch.save(cpu_state_dict(trainer.model), os.path.join(model_dir, "best_model.pth"))
            best_raw_preds, best_val_labels = np.copy(raw), np.copy(lab)
            since = 0
        else:
            since += 1
            if since >= patience:                                    # train.py:350-352
                break
    out = {k: v[:done].tolist() for k, v in hist.items()}
    # the alert-level numbers of the reference's val_summary (val.py:178-218 -> utils.make_report) for the best epoch,
    # and the per-source policy metrics (val.py:381-614) when the candidate table is at hand
    from .val import alert_summary
    summary = alert_summary(best_raw_preds, best_val_labels) if best_raw_preds is not None else {}
    if val_cand is not None and best_raw_preds is not None:
        summary["policy_performance"] = policy_summary(val_cand, best_raw_preds, best_val_labels,
                                                       next(trainer.model.parameters()).device)
    if main:
        with open(os.path.join(model_dir, "report.json"), "w") as f:
            json.dump({"train_config": dict(config or {}), "Training history": out, "val_summary": summary}, f,
                      indent=2)
        if diagnostic and val_cand is not None and best_raw_preds is not None:
            from .diagnostics import cand_diagnostic_data, save_diagnostic_fig
            curves = {"loss": out["train_loss"], "val_loss": out["val_loss"], "accuracy": out["train_accuracy"],
                      "val_accuracy": out["val_accuracy"]}
            data = cand_diagnostic_data(val_cand, best_raw_preds, best_val_labels, history=curves,
                                        device=next(trainer.model.parameters()).device)
            with open(os.path.join(model_dir, "diagnostic.json"), "w") as f:
                json.dump(data, f)
            save_diagnostic_fig(data, model_dir, os.path.join(model_dir, f"{run_name}.pdf"))
    out["best_raw_preds"], out["best_val_labels"] = best_raw_preds, best_val_labels
    out["val_summary"] = summary
    return out


def policy_summary(cand, raw_preds, labels, device="cuda") -> dict:
    """``val.policy_performance`` for a candidate table: ``cand["objectId"]`` (names or integers), ``cand["jd"]``,
    ``cand["magpsf"]``, one row per alert in the order of ``raw_preds`` / ``labels``; the optional columns ``junk``,
    ``save_time`` and ``trigger_time`` are passed on when the table has them."""
    import numpy as np
    from .val import policy_performance
    _, ids = np.unique(np.asarray(cand["objectId"]), return_inverse=True)
    n = len(ids)
    raw_preds, labels = np.asarray(raw_preds).reshape(-1), np.asarray(labels).reshape(-1)
    if len(raw_preds) != n or len(labels) != n:
        raise ValueError(f"the candidate table has {n} rows for {len(raw_preds)} scores and {len(labels)} labels")
    dev = torch.device(device)
    extra = {k: torch.as_tensor(np.asarray(cand[k], dtype=bool if k == "junk" else np.float64)).to(dev)
             for k in ("junk", "save_time", "trigger_time") if k in cand}
    return policy_performance(torch.as_tensor(ids.astype(np.int64)).to(dev),
                              torch.as_tensor(np.asarray(cand["jd"], dtype=np.float64)).to(dev),
                              torch.as_tensor(np.asarray(cand["magpsf"], dtype=np.float64)).to(dev),
                              torch.as_tensor(labels.astype(np.int64)).to(dev),
                              torch.as_tensor(raw_preds.astype(np.float32)).to(dev), **extra)


def cluster_config(clu) -> dict:
    """``config['embedding_clusters']`` checked and completed.  ``"algorithm": "dbscan"`` (the default) takes ``eps``
    (required), ``min_samples`` (5); ``"hdbscan"`` takes ``min_cluster_size`` (5) and ``min_samples`` (None: the same)
    and no ``eps``, and ``outlier_scores`` (a bool; the result holds the key only when it is given and true); both take
    ``on`` (``"map"`` or ``"embedding"``) and ``method`` (``"tiles"`` or ``"grid"``)."""
    algorithm = clu.get("algorithm", "dbscan") if isinstance(clu, dict) else None
    own = {"dbscan": {"eps", "min_samples"},
           "hdbscan": {"min_cluster_size", "min_samples", "outlier_scores"}}.get(algorithm, set())
    unknown = set(clu) - own - {"algorithm", "on", "method"} if isinstance(clu, dict) else {"?"}
    if (unknown or algorithm not in ("dbscan", "hdbscan") or (algorithm == "dbscan" and "eps" not in clu)
            or not isinstance(clu.get("outlier_scores", False), bool)
            or clu.get("on", "map") not in ("map", "embedding") or clu.get("method", "tiles") not in ("tiles", "grid")):
        raise ValueError("config['embedding_clusters'] is a dict with the keys eps, min_samples, on "
                         "('map' or 'embedding') and method ('tiles' or 'grid') -- or, with algorithm = 'hdbscan', "
                         "min_cluster_size, min_samples and outlier_scores (a bool) in place of eps --, "
                         f"got {clu!r}")
    tail = dict(on=clu.get("on", "map"), method=clu.get("method", "tiles"))
    if algorithm == "dbscan":
        return dict(algorithm=algorithm, eps=float(clu["eps"]), min_samples=int(clu.get("min_samples", 5)), **tail)
    ms = clu.get("min_samples")
    if clu.get("outlier_scores"):
        tail["outlier_scores"] = True
    return dict(algorithm=algorithm, min_cluster_size=int(clu.get("min_cluster_size", 5)),
                min_samples=None if ms is None else int(ms), **tail)


def _cluster_rows(rows, clu: dict):
    """(labels, membership probabilities or None, GLOSH outlier scores or None) of ``rows`` by a checked
    ``cluster_config``"""
    if clu["algorithm"] == "hdbscan":
        from .hdbscan import hdbscan
        labels, prob, tree = hdbscan(rows, clu["min_cluster_size"], clu["min_samples"], method=clu["method"],
                                     return_tree=True)
        return labels, prob, tree.outlier_scores(clu["min_cluster_size"]) if clu.get("outlier_scores") else None
    from .clusters import dbscan
    return dbscan(rows, clu["eps"], clu["min_samples"], method=clu["method"])[0], None, None


def write_embeddings(model, config: dict, data_base_dir: str, model_dir: str, stem: str, batch_size: int = 1024,
                     device="cuda", layer: str = "features") -> str:
    """The embedding step at the end of a run (train.py:449-469, whose helper module the reference does not ship): load
    ``model_dir/best_model.pth`` into ``model``, embed every alert of the test split -- of the validation split when
    there are no test files -- through ``ScoreStream(embed=layer)`` and write ``{stem}.npy`` (fp32 [N, width], rows in
    the candidate file's order) and, when that file has a ``candid`` column, ``{stem}.csv`` with it.  With
    ``config['embedding_neighbors'] = k`` also ``{stem}_knn.npz``: ``indices`` int64 [N, k] and ``distances`` fp32 [N, k] of ``knn_graph(rows, k,
    include_self=True)`` (the layout umap-learn's ``precomputed_knn`` takes) and ``candid`` where the table has it; with
    the dict ``{"k": 15, "group_by": "objectId", "mode": "exclude"}`` the graph of ``knn_graph(..., groups=ids,
    group_mode=mode)``, ``ids = alert_utils.object_keys`` of that column (an error names a column the table lacks), and
    ``groups`` = these ids in the file.  ``config['embedding_layout']`` takes ``"group_by"`` likewise (``groups=ids``).
    With ``config['embedding_novelty'] = k`` (or the same dict form) also ``{stem}_lof.npy``: float64 [N], the local
    outlier factor of every row among the others (``novelty.local_outlier_factor(rows, k, groups=ids, group_mode=mode)``).
    With ``config['embedding_layout']`` (``True``, or a dict of ``embedding_layout`` keyword arguments; ``seed`` defaults
    to the run's ``random_seed``) also ``{stem}_umap.csv`` with the reference's columns ``umap_emb_1, umap_emb_2,
    candid`` (train.py:464): the 2-D map of the rows, in the candidate file's order.  With
    ``config['embedding_clusters'] = {"eps": ..., "min_samples": 5, "on": "map" | "embedding", "method": "tiles" |
    "grid"}`` (``"grid"``: the 2-D map only, the same labels in time linear in the rows) the DBSCAN labels
    (``clusters.dbscan``; -1 = noise) of the map, as a ``cluster`` column of ``{stem}_umap.csv``, or of the embedding
    rows, as ``{stem}_clusters.npy`` (int64 [N]).  With ``"algorithm": "hdbscan"`` in that dict (``min_cluster_size``,
    ``min_samples`` in place of ``eps``; ``cluster_config``) the labels are ``hdbscan.hdbscan``'s and the membership
    strengths are left as ``{stem}_cluster_prob.npy`` (float64 [N]), and with ``"outlier_scores": True`` next to it the
    GLOSH scores as ``{stem}_cluster_outlier.npy`` (float64 [N]).  ``config['embedding_layout']`` also takes ``"quality": True | k``:
    ``write_map_quality`` leaves ``{stem}_umap_quality.json``, the map's trustworthiness, continuity and neighbour recall
    at ``k`` (``True``: the layout's ``n_neighbors``).  Returns the .npy path."""
    import numpy as np
    from .data import load_split
    from .pipeline import ScoreStream
    from .to_HF import strip_module_prefix
    dev = torch.device(device)
    state = torch.load(os.path.join(model_dir, "best_model.pth"), map_location="cpu")
    model.load_state_dict(strip_module_prefix(state), strict=True)
    model = model.to(dev).eval()
    try:
        images, metadata, _labels, cand = load_split(data_base_dir, config, "test")
    except FileNotFoundError:
        images, metadata, _labels, cand = load_split(data_base_dir, config, "val")
    parts = [t for t in (images, metadata) if t is not None]      # forward's own argument order
    n = parts[0].shape[0]
    batches = (tuple(t[i:i + batch_size].to(dev) for t in parts) for i in range(0, n, batch_size))
    rows = [emb.cpu() for _logits, emb in ScoreStream(model, embed=layer).map(batches)]
    out = torch.cat(rows).numpy() if rows else np.zeros((0, model.embedding_dim(layer)), dtype=np.float32)
    os.makedirs(os.path.dirname(stem) or ".", exist_ok=True)
    np.save(stem + ".npy", out)
    if "candid" in cand.columns:
        cand[["candid"]].to_csv(stem + ".csv", index=False)
    def group_ids(column, key):
        """int64 ids of the candidate table's ``column`` (alert_utils.object_keys) on ``dev``"""
        from .alert_utils import object_keys
        if column not in cand.columns:
            raise KeyError(f"config[{key!r}]['group_by'] = {column!r}: the candidate table has no such column "
                           f"(it has {list(cand.columns)})")
        return torch.from_numpy(object_keys(cand[column].to_numpy())).to(dev)

    k = config.get("embedding_neighbors")
    if k:   # opt-in: the neighbour search get_torch_embedding runs in front of its UMAP layout
        from .neighbors import knn_graph
        kw, extra = {}, {}
        if isinstance(k, dict):   # {"k": 15, "group_by": "objectId", "mode": "exclude"}: neighbours by source
            unknown = set(k) - {"k", "group_by", "mode"}
            if unknown or "k" not in k:
                raise ValueError(f"config['embedding_neighbors'] takes the keys k, group_by and mode, got {sorted(k)}")
            if k.get("group_by") is not None:
                kw = dict(groups=group_ids(k["group_by"], "embedding_neighbors"), group_mode=k.get("mode", "exclude"))
                extra["groups"] = kw["groups"].cpu().numpy()
            k = k["k"]
        idx, dist = knn_graph(torch.from_numpy(out).to(dev), int(k), include_self=True, **kw)
        if "candid" in cand.columns:
            extra["candid"] = cand["candid"].to_numpy()
        np.savez(stem + "_knn.npz", indices=idx.cpu().numpy(), distances=dist.cpu().numpy(), **extra)
    nov = config.get("embedding_novelty")
    if nov:   # opt-in: the local outlier factor of every row among the others ({stem}_lof.npy)
        from .novelty import local_outlier_factor
        kw = {}
        if isinstance(nov, dict):   # {"k": 20, "group_by": "objectId", "mode": "exclude"}: a row's own object left out
            unknown = set(nov) - {"k", "group_by", "mode"}
            if unknown or "k" not in nov:
                raise ValueError(f"config['embedding_novelty'] takes the keys k, group_by and mode, got {sorted(nov)}")
            if nov.get("group_by") is not None:
                kw = dict(groups=group_ids(nov["group_by"], "embedding_novelty"), group_mode=nov.get("mode", "exclude"))
            nov = nov["k"]
        lof = local_outlier_factor(torch.from_numpy(out).to(dev), int(nov), **kw)
        np.save(stem + "_lof.npy", lof.cpu().numpy())
    lay = config.get("embedding_layout")
    clu = config.get("embedding_clusters")
    if clu:   # opt-in: DBSCAN or HDBSCAN of the map (a `cluster` column of its table) or of the rows ({stem}_clusters.npy)
        clu = cluster_config(clu)
        if clu["on"] == "map" and not lay:
            raise ValueError("config['embedding_clusters'] with on='map' clusters the map of config['embedding_layout'], "
                             "which is not set")
        if clu["on"] == "embedding":
            labels, prob, glosh = _cluster_rows(torch.from_numpy(out).to(dev), clu)
            np.save(stem + "_clusters.npy", labels.cpu().numpy())
            if prob is not None:
                np.save(stem + "_cluster_prob.npy", prob.cpu().numpy())
            if glosh is not None:
                np.save(stem + "_cluster_outlier.npy", glosh.cpu().numpy())
    if lay:   # opt-in: the UMAP map itself, with the reference's columns (train.py:464)
        import pandas as pd
        from .layout import embedding_layout
        kw = dict(lay) if isinstance(lay, dict) else {}
        kw.setdefault("seed", int(config.get("random_seed", 0)))
        if kw.get("group_by") is not None:   # the map of the graph without the row's own object
            kw["groups"] = group_ids(kw["group_by"], "embedding_layout")
        kw.pop("group_by", None)
        quality = kw.pop("quality", None)   # True | k: judge the map (not an embedding_layout argument)
        emb_dev = torch.from_numpy(out).to(dev)
        y_dev = embedding_layout(emb_dev, **kw)
        if quality:
            write_map_quality(stem, emb_dev, y_dev, quality, kw)
        y = y_dev.cpu().numpy()
        table = {"umap_emb_1": y[:, 0], "umap_emb_2": y[:, 1]}
        if "candid" in cand.columns:
            table["candid"] = cand["candid"].to_numpy()
        if clu and clu["on"] == "map":
            labels, prob, glosh = _cluster_rows(y_dev, clu)
            table["cluster"] = labels.cpu().numpy()
            if prob is not None:
                np.save(stem + "_cluster_prob.npy", prob.cpu().numpy())
            if glosh is not None:
                np.save(stem + "_cluster_outlier.npy", glosh.cpu().numpy())
        pd.DataFrame(table).to_csv(stem + "_umap.csv", index=False)
    return stem + ".npy"


def write_map_quality(stem: str, emb, y, quality=True, layout_kw: Optional[dict] = None) -> str:
    """``quality.map_quality`` of the map ``y`` of the rows ``emb`` as ``{stem}_umap_quality.json``.  quality: ``True``
    (k = the layout's ``n_neighbors``, 15 by default) or k; layout_kw: the keyword arguments the map was laid out with,
    of which ``n_neighbors``, ``metric`` and ``groups`` are read.  Returns the path."""
    import json
    from . import quality as Q
    kw = layout_kw or {}
    k = kw.get("n_neighbors", 15) if quality is True else quality
    if isinstance(k, bool) or not isinstance(k, int):
        raise ValueError(f"config['embedding_layout']['quality'] must be True or an int k, got {quality!r}")
    res = Q.map_quality(emb, y, k, metric=kw.get("metric", "euclidean"), groups=kw.get("groups"))
    path = stem + "_umap_quality.json"
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    return path


def run_training(config: dict, data_base_dir: str = "", run_name: str = "testing", device="cuda",
                 precision: str = "bf16", models_root: str = "models", split_training: bool = False,
                 embeddings_root: str = "embeddings", diagnostic_fig: bool = False):
    """train.py:75-440 (``run_training(config)``) on this framework, minus WandB: seeds,
    the split files (``data.load_split``), the model by name with the frozen_fusion freezing rule
    (train.py:224-236), AdamW(lr, betas=(beta_1, beta_2)) under the warm-up + cosine schedule, BCE with
    pos_weight = N_neg / N_pos of the training split (train.py:211-212), the epoch loop with latest / best
    checkpoints and early stopping (``fit``), and the report, whose ``val_summary`` carries the per-source ``policy_performance`` when the validation
    split's candidate table has ``objectId``, ``jd`` and ``magpsf`` columns.  Under ``torch.distributed`` (one process per GPU,
    launched by torchrun) every rank trains its contiguous shard of each global batch and the gradients meet in one
    all-reduce per step; rank 0 writes the files.  Config keys are the reference's: model_name, epochs,
    batch_size, learning_rate, warmup_epochs, beta_1, beta_2, patience, random_seed, train_data_version, N_max,
    metadata_cols, data_aug_*, plus the model's own.  split_training: precision 'f16x2' with a ConvNeXt image branch
    only -- the training step's matrix products on split f16 operands (``set_split_training``).
    ``config['generate_embeddings']`` (train.py:449-469): after the best checkpoint is chosen, ``write_embeddings``
    leaves ``{embeddings_root}/{model_name}_{run_name}.npy`` (+ ``.csv``); a failure there is printed and the run
    still returns, as in the reference.  ``diagnostic_fig`` (train.py:378, off by default): when the validation table
    has the light-curve columns, rank 0 leaves ``diagnostic.json`` and, with matplotlib, ``{run_name}.pdf`` in the model
    directory (``fit``'s ``diagnostic``).  Returns (history dict, model_dir)."""
    import numpy as np
    import torch.distributed as dist
    from . import architectures
    from .data import DeviceDataset, load_split
    model_name = config["model_name"]
    epochs, batch_size = int(config["epochs"]), int(config["batch_size"])
    lr = float(config["learning_rate"])                    # "sometimes WandB makes LR a string" (train.py:85)
    warmup = int(config.get("warmup_epochs", 0))
    betas = (float(config["beta_1"]), float(config["beta_2"]))
    patience, seed = int(config["patience"]), int(config["random_seed"])
    version, n_str = config["train_data_version"], f"_N{config.get('N_max', 100)}"
    dev = torch.device(device)
    world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
    rank = dist.get_rank() if world > 1 else 0
    np.random.seed(seed)
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)
    timg, tmeta, tlab, _ = load_split(data_base_dir, config, "train")
    vimg, vmeta, vlab, vcand = load_split(data_base_dir, config, "val")
    if not all(c in vcand.columns for c in ("objectId", "jd", "magpsf")):   # no light curves: the alert-level summary alone
        vcand = None
    try:
        model_type = getattr(architectures, model_name)
    except AttributeError:
        raise ValueError(f"Could not find model of name {model_name}") from None
    model = model_type(config, precision=precision)
    if split_training:
        model.set_split_training(True)
    model = model.to(dev).train()
    if model_name == "frozen_fusion":                      # only the combined head is trained
        for p in list(model.image_branch.parameters()) + list(model.meta_branch.parameters()):
            p.requires_grad = False
        for p in model.combined_head.parameters():
            p.requires_grad = True
        for m in model._image_bn_modules():                # a MaxViT branch is served in eval mode only
            m.eval()
    else:
        for p in model.parameters():
            p.requires_grad = True
    gen = torch.Generator(device=dev).manual_seed(seed)    # the same permutations on every rank
    train_set = DeviceDataset(timg, tmeta, tlab, batch_size, config=config, device=dev, generator=gen,
                              shard=(rank, world) if world > 1 else None)
    trainer = Trainer(model, lr=lr, betas=betas, pos_weight=train_set.pos_weight, epochs=epochs,
                      warmup_epochs=warmup)
    model_dir = os.path.join(models_root, f"{model_name}_{version}{n_str}_{dev.type}", run_name) + "/"
    hist = fit(trainer, train_set, vimg, vmeta, vlab, model_dir, epochs=epochs, patience=patience,
               val_batch_size=batch_size, config=config, val_cand=vcand, diagnostic=diagnostic_fig,
               run_name=run_name)
    if config.get("generate_embeddings", False) and rank == 0:
        try:
            hist["embeddings_file"] = write_embeddings(model, config, data_base_dir, model_dir,
                                                       os.path.join(embeddings_root, f"{model_name}_{run_name}"),
                                                       batch_size=batch_size, device=dev)
        except Exception as e:                             # train.py:466-469
            import traceback
            print("Error generating embeddings", e)
            print(traceback.format_exc())
            print("Skipping embedding generation.")
    return hist, model_dir
