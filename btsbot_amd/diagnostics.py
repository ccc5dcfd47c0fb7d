"""The reference's diagnostic figure (btsbot/val.py:173-682 there, ``diagnostic_fig``): the data of its twelve
panels from the device, and the figure drawn from that data.

``alert_histograms`` is ``btsbot_alert_histograms`` behind tensors: one pass over a split's alerts gives the score /
magnitude density with its two marginals, the TP / FP / TN / FN counts per half-magnitude bin and the confusion counts.
``roc_points`` is sklearn's ``roc_curve`` restated: a sort and scans on the device, the two divisions on the host.
``diagnostic_data`` puts these next to ``val.alert_summary`` and ``val.policy_performance`` and adds the per-object
``save_dt`` values behind the last row of panels; ``draw_diagnostic_fig`` is matplotlib alone and never touches torch;
``diagnostic_fig`` has the reference's name and arguments.

Bin rule everywhere (numpy's, which the reference's figure goes through): bin i holds ``edges[i] <= x < edges[i+1]``, the
last bin also ``x == edges[-1]``; anything else, NaN included, is dropped.  Scores are compared as the float32 value
widened to float64, as ``val.policy_eval`` does.
"""
from __future__ import annotations

import ctypes as C
import os
import warnings
from typing import Dict, Mapping, Optional

import numpy as np
import torch

from . import _lib
from .val import (REFERENCE_POLICIES, _alert_summary_device, _alert_summary_dict, _policy_performance_device,
                  _policy_performance_dict)

HIST_MAX_BINS = 64            # per table (MAXB in csrc/alert_hist.hip)
HIST_MAX_JOINT = 4096         # n_mag * n_score
CLASSES = ("TP", "FP", "TN", "FN")
SAVE_DT_BINS = 50             # st_ax.hist(..., bins=50), val.py:596
_DRAWN_POLICIES = 3           # the reference has axes for its first three policies (val.py:422-423)


def _edges(bins, rng, name: str) -> np.ndarray:
    """``bins`` an integer: ``np.linspace(lo, hi, bins + 1)`` as np.histogram / np.histogram2d build them; an array: the
    caller's edges.  Finite, strictly increasing, 1..64 bins."""
    if np.ndim(bins) == 0:
        nb = int(bins)
        if nb != bins or not 1 <= nb <= HIST_MAX_BINS:
            raise ValueError(f"{name}_bins must be an integer in 1..{HIST_MAX_BINS} or an array of edges, got {bins!r}")
        lo, hi = (float(v) for v in rng)
        e = np.linspace(lo, hi, nb + 1)
    else:
        e = np.array(bins, dtype=np.float64)
        if e.ndim != 1 or not 2 <= e.shape[0] <= HIST_MAX_BINS + 1:
            raise ValueError(f"{name}_bins must hold 2..{HIST_MAX_BINS + 1} edges, got shape {e.shape}")
    if not np.isfinite(e).all() or not (np.diff(e) > 0).all():
        raise ValueError(f"{name} edges must be finite and strictly increasing, got {e!r}")
    return np.ascontiguousarray(e)


def _hist_counts(magpsf, raw_preds, labels, me, se, ce, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The launch: int64 [n_mag * n_score + n_mag + n_score + 4 * n_class + 4] on the inputs' device, ``out`` added into."""
    for name, t in (("magpsf", magpsf), ("raw_preds", raw_preds), ("labels", labels)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a tensor, got {type(t).__name__}")
    if magpsf.device.type != "cuda":
        raise RuntimeError("btsbot_amd.diagnostics.alert_histograms runs on the GPU; there is no CPU "
                           f"fallback (magpsf is on {magpsf.device})")
    dev = magpsf.device
    n = magpsf.shape[0] if magpsf.dim() == 1 else -1
    for name, t in (("magpsf", magpsf), ("raw_preds", raw_preds), ("labels", labels)):
        if t.dim() != 1 or t.shape[0] != n:
            raise ValueError(f"{name} must be [{max(n, 0)}], got {tuple(t.shape)}")
    nm, ns, nc = len(me) - 1, len(se) - 1, len(ce) - 1
    if nm * ns > HIST_MAX_JOINT:
        raise ValueError(f"mag_bins * score_bins must be <= {HIST_MAX_JOINT}, got {nm} x {ns}")
    size = nm * ns + nm + ns + 4 * nc + 4
    if out is None:
        out = torch.zeros(size, dtype=torch.int64, device=dev)
    elif out.dtype != torch.int64 or out.device != dev or out.dim() != 1 or out.shape[0] != size or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous int64 [{size}] on {dev}")
    mag = magpsf.to(torch.float64).contiguous()
    raw = raw_preds.to(device=dev, dtype=torch.float32).contiguous()
    lab = labels.to(device=dev, dtype=torch.int32).contiguous()
    dp = C.POINTER(C.c_double)
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(_lib.lib().btsbot_alert_histograms(
            C.c_void_p(mag.data_ptr()), C.c_void_p(raw.data_ptr()), C.c_void_p(lab.data_ptr()), n,
            me.ctypes.data_as(dp), nm, se.ctypes.data_as(dp), ns, ce.ctypes.data_as(dp), nc,
            C.c_void_p(out.data_ptr()), C.c_void_p(st)), "btsbot_alert_histograms")
    return out


def _hist_views(out: torch.Tensor, nm: int, ns: int, nc: int) -> Dict[str, torch.Tensor]:
    o1, o2, o3 = nm * ns, nm * ns + nm, nm * ns + nm + ns
    return {"joint": out[:o1].view(nm, ns), "mag": out[o1:o2], "score": out[o2:o3],
            "cls": out[o3:o3 + 4 * nc].view(4, nc), "total": out[o3 + 4 * nc:]}


def alert_histograms(magpsf: torch.Tensor, raw_preds: torch.Tensor, labels: torch.Tensor, mag_bins=28, mag_range=(16, 21),
                     score_bins=28, score_range=(0, 1), class_bins=np.arange(15, 21.5, 0.5),
                     out: Optional[torch.Tensor] = None) -> dict:
    """Every alert-level count of the diagnostic figure, in one launch on the inputs' device.

    magpsf is taken as float64, raw_preds (the sigmoid scores) as float32, labels as 0/1 integers.  ``mag_bins`` /
    ``score_bins``: a bin count over ``mag_range`` / ``score_range`` (edges ``np.linspace(lo, hi, bins + 1)``, numpy's
    own) or an array of edges; ``class_bins``: an array of edges (or a count over ``mag_range``).  At most 64 bins per
    table and 4096 cells in the joint histogram; the edges are checked on the host (finite, strictly increasing) before
    anything is launched.  Returns int64 tensors on the device

    ``joint`` [n_mag, n_score] (magnitude AND score inside their ranges), ``mag`` [n_mag], ``score`` [n_score] (each on its
    own: not sums of ``joint``), ``cls`` [4, n_class] (rows TP, FP, TN, FN; ``pred = raw > 0.5``), ``total`` [4] (every
    alert, whatever its magnitude), ``counts`` (the flat buffer the others are views of)

    and the float64 numpy edges ``mag_edges``, ``score_edges``, ``class_edges``.  ``out``: a ``counts`` buffer of an
    earlier call with the same bins, added into (a split counted in pieces).  No host synchronisation."""
    me, se = _edges(mag_bins, mag_range, "mag"), _edges(score_bins, score_range, "score")
    ce = _edges(class_bins, mag_range, "class")
    counts = _hist_counts(magpsf, raw_preds, labels, me, se, ce, out)
    res = _hist_views(counts, len(me) - 1, len(se) - 1, len(ce) - 1)
    res.update(counts=counts, mag_edges=me, score_edges=se, class_edges=ce)
    return res


# ---- ROC -------------------------------------------------------------------------------------------------------------
def _compact(mask: torch.Tensor, cols) -> list:
    """The rows of every column where ``mask`` holds, moved to the front of a buffer of len(mask) + 1 (the rest is
    scratch): a scan and a scatter, no size is read."""
    n = mask.shape[0]
    dest = torch.where(mask, torch.cumsum(mask, 0) - 1, torch.full_like(mask, n, dtype=torch.int64))
    return [torch.zeros(n + 1, dtype=c.dtype, device=c.device).scatter_(0, dest, c) for c in cols]


def _roc_device(raw_preds: torch.Tensor, labels: torch.Tensor):
    """sklearn's ``roc_curve`` (defaults) up to its divisions, without a host read: int64 [3, n + 2] whose first ``count``
    columns are (tps, fps, the bits of the float64 threshold) at the kept points, origin not included, and ``count`` (a
    device scalar)."""
    p = raw_preds.reshape(-1).to(torch.float64)
    y = (labels.reshape(-1).to(p.device) == 1).to(torch.int64)
    n = p.shape[0]
    score, order = torch.sort(p, descending=True, stable=True)
    tps = torch.cumsum(y[order], 0)
    fps = torch.arange(1, n + 1, device=p.device) - tps
    last = torch.ones(n, dtype=torch.bool, device=p.device)          # the last alert of every distinct score
    last[:-1] = score[1:] != score[:-1]
    tps, fps, thr = _compact(last, (tps, fps, score.view(torch.int64)))
    k = last.sum()
    # drop_intermediate: an interior point stays when fps or tps bends there (a non-zero second difference)
    j = torch.arange(n + 1, device=p.device)
    bend = torch.zeros(n + 1, dtype=torch.bool, device=p.device)
    if n >= 3:
        bend[1:-1] = ((fps[2:] - 2 * fps[1:-1] + fps[:-2]) != 0) | ((tps[2:] - 2 * tps[1:-1] + tps[:-2]) != 0)
    keep = (j < k) & ((j == 0) | (j == k - 1) | bend)
    return torch.stack(_compact(keep, (tps, fps, thr))), keep.sum()


def _trapezoid(y: np.ndarray, x: np.ndarray) -> float:
    return float(np.sum(np.diff(x) * (y[1:] + y[:-1]) / 2.0))


def _roc_host(tps: np.ndarray, fps: np.ndarray, thr: np.ndarray) -> dict:
    """The host end of ``roc_curve``: the origin in front, the two divisions in float64, the trapezoid area."""
    tps, fps = np.r_[0, tps].astype(np.float64), np.r_[0, fps].astype(np.float64)
    thr = np.r_[np.inf, thr]
    nan = np.full(len(tps), np.nan)
    fpr = fps / fps[-1] if fps[-1] > 0 else nan                      # no negatives: a NaN column, as sklearn
    tpr = tps / tps[-1] if tps[-1] > 0 else nan.copy()
    auc = _trapezoid(tpr, fpr) if len(fpr) >= 2 else float("nan")
    return {"fpr": fpr, "tpr": tpr, "thresholds": thr, "auc": auc}


def roc_points(raw_preds: torch.Tensor, labels: torch.Tensor) -> dict:
    """``sklearn.metrics.roc_curve(labels, raw_preds)`` with its defaults, and the area under it: a stable descending
    sort on the device, one point per distinct score with the cumulative true and false positives, the interior points
    where neither count bends dropped (``drop_intermediate``), the origin with threshold ``inf`` in front.  The integer
    counts at the kept points are made by torch ops on the scores' device and read ONCE (the buffers padded to the alert
    count, so that no size has to be read first); ``fpr = fps / fps[-1]`` and ``tpr = tps / tps[-1]`` are float64
    numpy on the host, bit for bit sklearn's.  Without a negative (positive) ``fpr`` (``tpr``) is all NaN, and so is
    ``auc``.  Returns ``{"fpr", "tpr", "thresholds"}`` as float64 numpy arrays and ``"auc"`` (the trapezoid rule)."""
    for name, t in (("raw_preds", raw_preds), ("labels", labels)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a tensor, got {type(t).__name__}")
    if raw_preds.numel() != labels.numel():
        raise ValueError("raw_preds / labels length mismatch")
    if raw_preds.numel() == 0:
        return _roc_host(np.zeros(0), np.zeros(0), np.zeros(0))
    pts, count = _roc_device(raw_preds, labels)
    flat = torch.cat([pts.reshape(-1), count.reshape(1)]).cpu().numpy()          # the one host read
    k = int(flat[-1])
    pts = flat[:-1].reshape(3, -1)[:, :k]
    return _roc_host(pts[0], pts[1], np.ascontiguousarray(pts[2]).view(np.float64))


# ---- the panels' data ------------------------------------------------------------------------------------------------
def _save_dt_hist(values: np.ndarray) -> Optional[dict]:
    """What ``st_ax.hist(save_dt, bins=50)`` draws: 50 equal bins over [min, max] of the values there are."""
    if values.size == 0:
        return None
    counts, edges = np.histogram(values, bins=SAVE_DT_BINS, range=(values.min(), values.max()))
    return {"values": values.tolist(), "counts": counts.tolist(), "edges": edges.tolist()}


def diagnostic_data(object_id: torch.Tensor, jd: torch.Tensor, magpsf: torch.Tensor, label: torch.Tensor,
                    raw_preds: torch.Tensor, junk: Optional[torch.Tensor] = None,
                    save_time: Optional[torch.Tensor] = None, trigger_time: Optional[torch.Tensor] = None,
                    policies: Mapping = REFERENCE_POLICIES, history: Optional[Mapping] = None) -> dict:
    """Everything the twelve panels of the reference's diagnostic figure show, as JSON-serialisable lists and floats.

    The arguments are ``val.policy_performance``'s, device tensors with one row per alert; ``history`` (``loss``,
    ``val_loss``, ``accuracy``, ``val_accuracy`` per epoch, any of them) is passed through for the first two panels.

    ``roc``: ``fpr``, ``tpr``, ``thresholds``, ``auc`` (``roc_points``).  ``score_mag_hist``: ``counts`` [28][28]
    (magnitude bin, score bin), ``mag_edges``, ``score_edges``, ``mag_counts``, ``score_counts``.  ``class_mag_hist``:
    ``bins`` (13 edges) and ``TP``, ``FP``, ``TN``, ``FN`` per bin.  ``confusion``: the four counts and ``normalized``,
    [[TN, FP], [FN, TP]] over the true label's row sum (an empty row: zeros), as the panel shows it.  ``summary``:
    ``val.alert_summary``'s dict.  ``history``.  ``policy_performance``: exactly ``val.policy_performance``'s dict.
    ``policy_save_dt``: per policy ``{"values", "counts", "edges"}`` -- the ``save_dt`` of the true-positive objects with
    a trusted save time and a trigger (the values ``med_save_dt`` is the median of), and their histogram in 50 equal
    bins over [min, max] -- or None when there is no value (no ``save_time``; no true positive or no true negative).

    All the device work is queued first: the histogram launch, the ROC sort and scans, the summary's sums, the policy
    kernel and its reductions.  Then the host reads TWICE: once everything of fixed size together with the two sizes
    that are not known before (kept ROC points, object slots), once the ROC points and the ``save_dt`` columns cut to
    those sizes."""
    me, se = _edges(28, (16, 21), "mag"), _edges(28, (0, 1), "score")
    ce = _edges(np.arange(15, 21.5, 0.5), None, "class")
    nm, ns, nc = len(me) - 1, len(se) - 1, len(ce) - 1
    names, rows, save_dt = _policy_performance_device(object_id, jd, magpsf, label, raw_preds, policies, junk, save_time,
                                                      trigger_time)                  # (validates the columns)
    dev, n = object_id.device, object_id.shape[0]
    counts = _hist_counts(magpsf, raw_preds, label, me, se, ce)
    if n:
        summary = _alert_summary_device(raw_preds.to(dev), label)
        pts, n_roc = _roc_device(raw_preds.to(dev), label)
    else:
        summary = torch.zeros(7, dtype=torch.float64, device=dev)
        pts, n_roc = torch.zeros((3, 1), dtype=torch.int64, device=dev), torch.zeros((), dtype=torch.int64, device=dev)
    if save_dt is not None and n:
        dt_sorted = torch.sort(save_dt, dim=0).values                               # NaN last: the values lead each column
        n_dt = (~torch.isnan(save_dt)).sum(0).max()
    else:
        dt_sorted = torch.zeros((1, len(names)), dtype=torch.float64, device=dev)
        n_dt = torch.zeros((), dtype=torch.int64, device=dev)
    fixed = torch.cat([counts.to(torch.float64), summary, rows.reshape(-1), n_roc.reshape(1).to(torch.float64),
                       n_dt.reshape(1).to(torch.float64)]).cpu().numpy()             # host read 1 (counts < 2^53: exact)
    n_roc, n_dt = int(fixed[-2]), int(fixed[-1])
    tail = torch.cat([pts[:, :n_roc].reshape(-1), dt_sorted[:n_dt].reshape(-1).view(torch.int64)]).cpu().numpy()  # read 2
    pts = tail[:3 * n_roc].reshape(3, n_roc)
    dts = tail[3 * n_roc:].view(np.float64).reshape(n_dt, len(names))
    size = counts.shape[0]
    h = {k: v.numpy() for k, v in _hist_views(torch.from_numpy(fixed[:size].astype(np.int64)), nm, ns, nc).items()}
    roc = _roc_host(pts[0], pts[1], np.ascontiguousarray(pts[2]).view(np.float64))
    perf = _policy_performance_dict(names, fixed[size + 7:-2].reshape(len(names), -1).tolist())
    tp, fp, tn, fn = (int(v) for v in h["total"])
    save = {}
    for q, name in enumerate(names):
        col = dts[:, q]
        ok = perf[name]["policy_precision"] != -999.0                                # (the reference draws nothing then)
        save[name] = _save_dt_hist(col[~np.isnan(col)]) if ok else None
    return {
        "roc": {"fpr": roc["fpr"].tolist(), "tpr": roc["tpr"].tolist(), "thresholds": roc["thresholds"].tolist(),
                "auc": roc["auc"]},
        "score_mag_hist": {"counts": h["joint"].tolist(), "mag_edges": me.tolist(), "score_edges": se.tolist(),
                           "mag_counts": h["mag"].tolist(), "score_counts": h["score"].tolist()},
        "class_mag_hist": dict({"bins": ce.tolist()}, **{c: h["cls"][i].tolist() for i, c in enumerate(CLASSES)}),
        "confusion": {"TP": tp, "FP": fp, "TN": tn, "FN": fn,
                      "normalized": [[tn / (tn + fp), fp / (tn + fp)] if tn + fp else [0.0, 0.0],
                                     [fn / (fn + tp), tp / (fn + tp)] if fn + tp else [0.0, 0.0]]},
        "summary": _alert_summary_dict(fixed[size:size + 7].tolist()),
        "history": {k: [float(v) for v in history[k]] for k in ("loss", "val_loss", "accuracy", "val_accuracy")
                    if history is not None and k in history},
        "policy_performance": perf,
        "policy_save_dt": save,
    }


# ---- the figure ------------------------------------------------------------------------------------------------------
_warned_no_matplotlib = False


def _matplotlib():
    """matplotlib.pyplot on the Agg backend, or None (with one warning per process) where it is not installed."""
    global _warned_no_matplotlib
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
        return plt
    except ImportError:
        if not _warned_no_matplotlib:
            warnings.warn("matplotlib is not installed: the diagnostic figure is not drawn (its data is returned)")
            _warned_no_matplotlib = True
        return None


def draw_diagnostic_fig(data: Mapping, title: str = ""):
    """The reference's 4 x 3 figure (val.py:229-668) from ``diagnostic_data``'s dict: accuracy and loss histories, ROC;
    score / magnitude density with its marginals, confusion matrix, TP / FP / TN / FN by magnitude; purity and
    completeness of the first three policies; their days gained on the scanners.  matplotlib alone (Agg, imported
    here): no torch and no GPU call.  Returns the Figure."""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.gridspec as gridspec
    import matplotlib.pyplot as plt
    import matplotlib.ticker as mtick
    from matplotlib.colors import LogNorm
    from mpl_toolkits.axes_grid1 import make_axes_locatable

    summary, hist, roc = data["summary"], data.get("history") or {}, data["roc"]
    fig = plt.figure(figsize=(20, 22), dpi=200)
    grid = gridspec.GridSpec(4, 3, wspace=0.3, hspace=0.3)
    fig.suptitle(title, size=28, y=0.92)

    ax1 = fig.add_subplot(grid[0])
    ax1.plot(hist.get("accuracy", []), label="Training", linewidth=2)
    ax1.plot(hist.get("val_accuracy", []), label="Validation", linewidth=2)
    for key, name, colour in (("bts_acc", "BTS", "blue"), ("notbts_acc", "notBTS", "green"), ("bal_acc", "Balanced", "gray")):
        if np.isfinite(summary[key]):
            ax1.axhline(summary[key], label=name, c=colour, linewidth=1.5, linestyle="dashed")
    ax1.set_xlabel("Epoch", size=18)
    ax1.set_ylabel("Accuracy", size=18)
    ax1.legend(loc="best")
    ax1.grid(True, linewidth=.3)

    ax2 = fig.add_subplot(grid[1])
    ax2.plot(hist.get("loss", []), label="Training", linewidth=2)
    ax2.plot(hist.get("val_loss", []), label="Validation", linewidth=2)
    ax2.set_xlabel("Epoch", size=18)
    ax2.set_ylabel("Loss", size=18)
    ax2.legend(loc="best")
    ax2.grid(True, linewidth=.3)

    ax3 = fig.add_subplot(grid[2])
    ax3.plot([0, 1], [0, 1], color="k", lw=2, linestyle="--")
    ax3.set_xlim([0.0, 1.0])
    ax3.set_ylim([0.0, 1.05])
    ax3.plot(roc["fpr"], roc["tpr"], lw=2, label=f"ROC (area = {roc['auc']:.5f})")
    ax3.set_xlabel("False Positive Rate (Contamination)")
    ax3.set_ylabel("True Positive Rate (Sensitivity)")
    ax3.legend(loc="lower right")
    ax3.grid(True, linewidth=.3)
    ax3.set(aspect="equal")

    # score against magnitude: the counted cells as the mesh hist2d would have drawn, the marginals as bars
    sm = data["score_mag_hist"]
    me, se = np.asarray(sm["mag_edges"]), np.asarray(sm["score_edges"])
    joint = np.asarray(sm["counts"], dtype=np.float64)
    ax4_grid = gridspec.GridSpecFromSubplotSpec(2, 2, subplot_spec=grid[3], width_ratios=[1, 6], height_ratios=[1, 6],
                                                hspace=0.05, wspace=0.05)
    ax4 = fig.add_subplot(ax4_grid[1, 1])
    ax4_histx = fig.add_subplot(ax4_grid[0, 1], sharex=ax4)
    ax4_histy = fig.add_subplot(ax4_grid[1, 0], sharey=ax4)
    norm = LogNorm() if joint.max(initial=0) > 0 else None
    mesh = ax4.pcolormesh(me, se, np.ma.masked_equal(joint, 0).T if norm else joint.T, norm=norm, cmap=plt.cm.viridis)
    ax4.set_xlim(me[0], me[-1])
    ax4.set_ylim(se[0], se[-1])
    ax4.set_aspect("auto")
    ax4.xaxis.set_major_locator(mtick.MultipleLocator(1))
    ax4.xaxis.set_minor_locator(mtick.MultipleLocator(0.5))
    ax4.set_xlabel("PSF Magnitude", size=22)
    ax4.yaxis.set_major_locator(mtick.MultipleLocator(0.2))
    ax4.yaxis.set_minor_locator(mtick.MultipleLocator(0.1))
    extend = make_axes_locatable(ax4).append_axes("right", "5%", pad=0.2)
    fig.colorbar(mesh, cax=extend)
    extend.set_ylabel("# of alerts", size=18)
    ax4_histx.bar(me[:-1], sm["mag_counts"], width=np.diff(me), align="edge", facecolor="#37125E")
    ax4_histx.tick_params(direction="out", axis="x", length=2, width=1, bottom=True, pad=10)
    ax4_histx.tick_params(axis="y", left=False, right=False)
    ax4_histx.set_yticklabels([])
    ax4_histy.barh(se[:-1], sm["score_counts"], height=np.diff(se), align="edge", facecolor="#37125E")
    ax4_histy.set_ylabel("Bright transient score", size=22)
    ax4_histy.tick_params(direction="out", axis="y", length=2, width=1, bottom=True, pad=10)
    ax4_histy.tick_params(axis="x", bottom=False)
    ax4_histy.set_xticklabels([])
    ax4_histy.invert_xaxis()
    ax4_histy.set_aspect("auto")
    for ax in (ax4, ax4_histx, ax4_histy):
        ax.label_outer()

    # confusion matrix, each row over its true label (ConfusionMatrixDisplay(normalize="true"))
    ax5 = fig.add_subplot(grid[4])
    cm = np.asarray(data["confusion"]["normalized"], dtype=np.float64)
    ax5.imshow(cm, cmap=plt.cm.Blues, vmin=0, vmax=1)
    for r in range(2):
        for c in range(2):
            ax5.text(c, r, f"{cm[r, c]:.2g}", ha="center", va="center", color="white" if cm[r, c] > 0.5 else "black")
    ax5.set_xticks([0, 1], ["notBTS", "BTS"])
    ax5.set_yticks([0, 1], ["notBTS", "BTS"])
    ax5.set_xlabel("Predicted label")
    ax5.set_ylabel("True label")

    ax6 = fig.add_subplot(grid[5])
    ch = data["class_mag_hist"]
    bins = np.asarray(ch["bins"])
    bottom = np.zeros(len(bins) - 1)
    for name, colour in zip(CLASSES, ("#26547C", "#A9BCD0", "#BA5A31", "#E59F71")):
        ax6.bar(bins[:-1], ch[name], bottom=bottom, align="edge", width=np.diff(bins), color=colour, label=name,
                linewidth=0.1, edgecolor="k")
        bottom = bottom + np.asarray(ch[name])
    ax6.axvspan(10, 18.5, color="gold", alpha=0.2, lw=0)
    ax6.legend(ncol=2, frameon=False)
    ax6.set_xlim([16, 21])
    ax6.xaxis.set_major_locator(mtick.MultipleLocator(1))
    ax6.xaxis.set_minor_locator(mtick.MultipleLocator(0.5))
    ax6.tick_params(direction="out", axis="x", length=2, width=1, bottom=True, pad=10)
    ax6.tick_params(axis="y", left=False, right=False)
    ax6.set_xlabel("PSF Magnitude", size=18)
    ax6.set_ylabel("# of alerts", size=18)

    cp_axes = [fig.add_subplot(grid[6 + q]) for q in range(_DRAWN_POLICIES)]
    st_axes = [fig.add_subplot(grid[9 + q]) for q in range(_DRAWN_POLICIES)]
    perf, save = data.get("policy_performance") or {}, data.get("policy_save_dt") or {}
    for name, cp_ax, st_ax in zip(perf, cp_axes, st_axes):
        p = perf[name]
        edges = np.asarray(p["peakmag_bins"])
        if p["policy_precision"] != -999.0:
            rec, pur = np.asarray(p["binned_recall"]), np.asarray(p["binned_precision"])
            cp_ax.step(edges, 100 * np.append(rec[0], rec), color="#263D65", label="Completeness", linewidth=3)
            cp_ax.step(edges, 100 * np.append(pur[0], pur), color="#FE7F2D", label="Purity", linewidth=3)
            cp_ax.axhline(100 * p["policy_precision"], color="#FE7F2D", linewidth=2, linestyle="dashed")
            cp_ax.axhline(100 * p["policy_recall"], color="#263D65", linewidth=2, linestyle="dashed")
            dt = save.get(name)
            if dt is not None:
                st_ax.stairs(dt["counts"], dt["edges"], edgecolor="#654690", linewidth=3, label=name + "_save")
        cp_ax.text(x=17.75, y=76.25, s=f"{name}\n({100 * p['policy_recall']:.0f}%,{100 * p['policy_precision']:.0f}%)",
                   fontsize=20, fontweight="bold", c="#654690")
        cp_ax.axvline(18.5, c="k", linewidth=1, linestyle="dashed", alpha=0.5, zorder=10)
        cp_ax.grid(True, linewidth=.3)
        cp_ax.set_xlim([17.0, 18.5])
        cp_ax.set_ylim([75, 100.5])
        cp_ax.xaxis.set_major_locator(mtick.MultipleLocator(0.5))
        cp_ax.xaxis.set_minor_locator(mtick.MultipleLocator(0.25))
        cp_ax.yaxis.set_major_locator(mtick.MultipleLocator(10))
        cp_ax.yaxis.set_minor_locator(mtick.MultipleLocator(5))
        cp_ax.yaxis.set_major_formatter(mtick.PercentFormatter(decimals=0))
        cp_ax.tick_params(direction="in", axis="both", length=3, width=1.5, bottom=True, left=True, right=True, pad=10)
        cp_ax.tick_params(which="minor", direction="in", axis="y", length=1.5, width=1.5, bottom=True, left=True,
                          right=True, pad=10)
        cp_ax.set_xlabel("Peak Magnitude", size=22)
        cp_ax.set_ylabel("% of objects", size=18)
        if np.isfinite(p["med_save_dt"]):
            st_ax.axvline(p["med_save_dt"], linestyle="solid", c="k", linewidth=1.5, label=f"med:\n{p['med_save_dt']:.2f} d")
        st_ax.axvline(0, linestyle="dashed", c="gray", linewidth=1)
        st_ax.set_xlim([-15, 15])
        st_ax.set_ylim([0, 55])
        st_ax.legend(prop={"size": 20}, frameon=False)
        st_ax.set_ylabel("# of sources", size=18)
        st_ax.set_xlabel("Days after save by scanner", size=22)
    cp_axes[0].axhline(0, color="gray", linewidth=2, linestyle="dashed", label="Overall")
    cp_axes[0].legend(prop={"size": 14}, frameon=False, loc="lower left")
    for ax in [ax1, ax2, ax3, ax4, ax5, ax6, extend] + cp_axes + st_axes:
        ax.tick_params(which="both", width=1.5)
    return fig


def _cand_columns(cand) -> dict:
    """A csv path or a table -> its columns (``train.policy_summary``'s convention)."""
    if isinstance(cand, (str, os.PathLike)):
        import pandas as pd
        cand = pd.read_csv(cand, index_col=None)
    missing = [c for c in ("objectId", "jd", "magpsf") if c not in cand]
    if missing:
        raise ValueError(f"the candidate table lacks the columns {missing}")
    return cand


def cand_diagnostic_data(cand, raw_preds, labels, history: Optional[Mapping] = None, device="cuda") -> dict:
    """``diagnostic_data`` for a candidate table (a csv path, a dict or a DataFrame with ``objectId``, ``jd``, ``magpsf``
    per alert in the order of ``raw_preds`` / ``labels``, optionally ``junk``, ``save_time``, ``trigger_time``)."""
    cand = _cand_columns(cand)
    _, ids = np.unique(np.asarray(cand["objectId"]), return_inverse=True)
    n = len(ids)
    raw_preds, labels = np.asarray(raw_preds).reshape(-1), np.asarray(labels).reshape(-1)
    if len(raw_preds) != n or len(labels) != n:
        raise ValueError(f"the candidate table has {n} rows for {len(raw_preds)} scores and {len(labels)} labels")
    dev = torch.device(device)
    extra = {k: torch.as_tensor(np.asarray(cand[k], dtype=bool if k == "junk" else np.float64)).to(dev)
             for k in ("junk", "save_time", "trigger_time") if k in cand}
    return diagnostic_data(torch.as_tensor(ids.astype(np.int64)).to(dev),
                           torch.as_tensor(np.asarray(cand["jd"], dtype=np.float64)).to(dev),
                           torch.as_tensor(np.asarray(cand["magpsf"], dtype=np.float64)).to(dev),
                           torch.as_tensor(labels.astype(np.int64)).to(dev),
                           torch.as_tensor(raw_preds.astype(np.float32)).to(dev), history=history, **extra)


def save_diagnostic_fig(data: Mapping, title: str, path: str) -> bool:
    """Draw ``data`` and write the PDF at ``path``; False (after one warning) where matplotlib is not installed."""
    plt = _matplotlib()
    if plt is None:
        return False
    fig = draw_diagnostic_fig(data, title)
    fig.savefig(path, bbox_inches="tight")
    plt.close(fig)
    return True


def diagnostic_fig(run_data: Mapping, cand, run_descriptor: str, device="cuda", draw: bool = True) -> dict:
    """The reference's ``diagnostic_fig(run_data, cand_dir, run_descriptor)`` (val.py:173-682).  ``run_data``:
    ``raw_preds``, ``labels``, ``run_name`` and optionally the per-epoch ``loss``, ``val_loss``, ``accuracy``,
    ``val_accuracy``.  ``cand``: the split's candidate csv, or a table, with ``objectId``, ``jd``, ``magpsf`` and
    optionally ``junk``, ``save_time``, ``trigger_time`` -- what the reference reads from fixed files (``trues.csv``,
    ``RCFJunk*.csv``) is a column here.  Returns the reference's dict -- ``roc_auc``, ``bal_acc``, ``bts_acc``,
    ``notbts_acc``, ``alert_precision``, ``alert_recall``, ``policy_performance`` -- plus ``"data"``
    (``diagnostic_data``'s dict); with ``draw`` and matplotlib at hand also ``"fig"``, saved as
    ``{run_descriptor}/{run_name}.pdf`` as there (without matplotlib: one warning, and the rest)."""
    data = cand_diagnostic_data(cand, run_data["raw_preds"], run_data["labels"], history=run_data, device=device)
    out = {k: data["summary"][k] for k in ("roc_auc", "bal_acc", "bts_acc", "notbts_acc", "alert_precision",
                                           "alert_recall")}
    out["roc_auc"] = data["roc"]["auc"]
    out["policy_performance"] = data["policy_performance"]
    out["data"] = data
    if draw and _matplotlib() is not None:
        fig = draw_diagnostic_fig(data, run_descriptor)
        os.makedirs(run_descriptor, exist_ok=True)
        fig.savefig(os.path.join(run_descriptor, f"{run_data['run_name']}.pdf"), bbox_inches="tight")
        out["fig"] = fig
    return out
