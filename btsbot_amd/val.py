"""Validation pass and scalar metrics on the device (/root/reference/btsbot/val.py:31-170).

``run_val_tensors`` is the evaluate loop of val.py:117-168 for a split that is already in memory:
forward in batches (no shuffling, no augmentation), then BCEWithLogitsLoss(pos_weight) over ALL logits
and the accuracy of ``sigmoid(logits) > 0.5`` -- accumulated by ``btsbot_eval_metrics`` without a
per-batch ``.item()``.  Returns what the reference returns: (loss, accuracy, raw_preds, labels), the
last two as numpy arrays.  The model object is reused (the reference re-instantiates it and reloads
``best_model.pth`` on every call, val.py:64-74).

``policy_performance`` is the per-source half of the reference's summary (val.py:381-614 inside ``diagnostic_fig``):
does a scanning policy ("two alerts scored above 0.5 and brighter than 19 mag", ...) save an object, at what purity and
completeness, and how long before the human scanners.  ``policy_eval`` is its per-object kernel
(``btsbot_policy_eval``) behind tensors; the object filter, the counts and the medians are torch reductions on the
device.  A policy is ``(thr, cut, k, gate)``; any number of them go in one call, so a threshold sweep is

    policy_performance(object_id, jd, magpsf, label, raw_preds,
                       policies={f"t{t:.2f}": (t, 19.0, 1, 18.5) for t in np.arange(0.05, 1.0, 0.05)})
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Mapping, Optional, Tuple

import torch

from . import _lib
from .alert_utils import OBJECT_TILE, _check_table, _group_by_object, _launch_grouped
from .data import DeviceDataset


def device_metrics(logits: torch.Tensor, labels: torch.Tensor, pos_weight: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """(mean BCE-with-logits loss, accuracy) as device scalars; logits [N] or [N,1], labels 0/1."""
    z = logits.reshape(-1).to(torch.float32).contiguous()
    y = labels.reshape(-1).to(device=z.device, dtype=torch.float32).contiguous()
    if z.device.type != "cuda":
        raise RuntimeError("btsbot_amd.val.device_metrics runs on the GPU; there is no CPU fallback")
    if z.numel() != y.numel():
        raise ValueError("logits / labels length mismatch")
    out = torch.zeros(2, dtype=torch.float32, device=z.device)
    with torch.cuda.device(z.device):
        st = torch.cuda.current_stream(z.device).cuda_stream
        _lib.check(_lib.lib().btsbot_eval_metrics(C.c_void_p(z.data_ptr()), C.c_void_p(y.data_ptr()),
                                                  float(pos_weight), z.numel(),
                                                  C.c_void_p(out.data_ptr()), C.c_void_p(st)),
                   "btsbot_eval_metrics")
    n = max(z.numel(), 1)
    return out[0] / n, out[1] / n


def run_val_tensors(model, images, metadata, labels, batch_size: int = 1024,
                    pos_weight: Optional[float] = None, device="cuda"):
    """val.py:117-168.  ``pos_weight`` defaults to N_neg / N_pos of this split (val.py:60-62)."""
    ds = DeviceDataset(images, metadata, labels, batch_size, device=device, shuffle=False,
                       drop_last=False, augment=False, check_nan=False)
    pw = ds.pos_weight if pos_weight is None else float(pos_weight)
    was_training = model.training
    model.eval()
    logits = []
    with torch.no_grad():
        for batch in ds:
            if ds.images is not None and ds.metadata is not None:
                logits.append(model(image_input=batch[0], metadata_input=batch[1]))
            else:
                logits.append(model(input_data=batch[0]))
    model.train(was_training)
    all_logits = torch.cat(logits, dim=0) if logits else torch.empty(0, 1, device=ds.device)
    loss, acc = device_metrics(all_logits, ds.labels, pw)
    raw_preds = torch.sigmoid(all_logits).squeeze(1).cpu().numpy()
    return loss.item(), acc.item(), raw_preds, ds.labels.float().cpu().numpy()


def alert_summary(raw_preds, labels) -> dict:
    """The alert-level part of the reference's validation summary (val.py:178-218; what train.py:404-411 logs and
    report.json keeps under ``val_summary``): confusion counts at the 0.5 threshold (``np.rint``: 0.5 rounds to 0),
    ``bts_acc`` / ``notbts_acc`` / ``bal_acc``, ``alert_precision`` / ``alert_recall`` (-999.0 when there is no true
    positive or no true negative, as there) and ``roc_auc`` (area under sklearn's ``roc_curve``: the rank statistic
    with tied scores sharing their average rank).  Everything is reduced on the tensors' device; one host read."""
    return _alert_summary_dict(_alert_summary_device(raw_preds, labels).cpu().tolist())   # the one host read


def _alert_summary_device(raw_preds, labels) -> torch.Tensor:
    """The seven sums ``alert_summary`` is made of, float64 on the inputs' device; nothing is read."""
    p = torch.as_tensor(raw_preds).reshape(-1).to(torch.float64)
    y = torch.as_tensor(labels, device=p.device).reshape(-1).to(torch.float64)
    if p.numel() != y.numel():
        raise ValueError("raw_preds / labels length mismatch")
    pred = torch.round(p)                                  # half-to-even, as np.rint
    tp = ((pred == 1) & (y == 1)).sum()
    tn = ((pred == 0) & (y == 0)).sum()
    fp = ((pred == 1) & (y == 0)).sum()
    fn = ((pred == 0) & (y == 1)).sum()
    # ROC AUC = P(score_pos > score_neg) + 0.5 P(tie): average ranks of the sorted scores
    order = torch.argsort(p, stable=True)
    ps = p[order]
    uniq, inv, cnt = torch.unique_consecutive(ps, return_inverse=True, return_counts=True)
    last = torch.cumsum(cnt, 0).to(torch.float64)          # rank of the last member of each tie group (1-based)
    avg_rank = (last - (cnt.to(torch.float64) - 1) / 2)[inv]
    n_pos, n_neg = y.sum(), (1 - y).sum()
    rank_sum = (avg_rank * y[order]).sum()
    return torch.stack([tp, tn, fp, fn, n_pos, n_neg, rank_sum]).to(torch.float64)


def _alert_summary_dict(vals) -> dict:
    tp, tn, fp, fn, n_pos, n_neg, rank_sum = vals
    nan = float("nan")
    bts_acc = tp / (tp + fn) if tp + fn > 0 else nan
    notbts_acc = tn / (tn + fp) if tn + fp > 0 else nan
    if tp > 0 and tn > 0:
        precision, recall = tp / (tp + fp), tp / (tp + fn)
    else:
        precision = recall = -999.0
    auc = (rank_sum - n_pos * (n_pos + 1) / 2) / (n_pos * n_neg) if n_pos > 0 and n_neg > 0 else nan
    return {"roc_auc": auc, "bal_acc": (bts_acc + notbts_acc) / 2, "bts_acc": bts_acc, "notbts_acc": notbts_acc,
            "alert_precision": precision, "alert_recall": recall,
            "TP": int(tp), "TN": int(tn), "FP": int(fp), "FN": int(fn)}


def run_val(config: dict, model_dir: str, model_filename: str, bts_weight: float, data_base_dir: str = "",
            split: str = "val", device="cuda", precision: str = "bf16"):
    """val.py:31-168 (``run_val(config, model_dir, model_filename, bts_weight, ...)``): instantiate the model the
    config names, load ``model_dir/model_filename`` strictly (a DataParallel ``module.`` prefix is accepted), read
    the split files and run the validation pass.  ``need_triplets`` / ``need_metadata`` follow from the model
    name as in train.py:108-122.  Returns (loss, accuracy, raw_preds, labels) like the reference."""
    import os
    from . import architectures
    from .data import load_split
    from .to_HF import strip_module_prefix
    try:
        model_type = getattr(architectures, config["model_name"])
    except AttributeError:
        raise ValueError(f"Could not find model of name {config['model_name']}") from None
    model = model_type(config, precision=precision)
    state = torch.load(os.path.join(model_dir, model_filename), map_location="cpu")
    model.load_state_dict(strip_module_prefix(state), strict=True)
    model = model.to(device).eval()
    images, metadata, labels, _ = load_split(data_base_dir, config, split)
    return run_val_tensors(model, images, metadata, labels, batch_size=int(config.get("batch_size", 1024)),
                           pos_weight=float(bts_weight), device=device)


# ---- per-object policy metrics (val.py:381-614) --------------------------------------------------------------------
# name -> (score threshold, magnitude cut, count, peak gate or None): the four policies the reference logs
REFERENCE_POLICIES = {"bts_p1": (0.5, 19.0, 2, None), "bts_p2": (0.5, 19.0, 2, 18.5),
                      "prod_p1": (0.85, 19.0, 1, None), "prod_p2": (0.85, 19.0, 1, 18.5)}
POLICY_TILE = OBJECT_TILE                                          # btsbot_policy_eval runs the shared per-object walk
POLICIES_PER_LAUNCH = 16
PEAKMAG_BINS = (17.0, 17.25, 17.5, 17.75, 18.0, 18.25, 18.5)       # np.arange(17.0, 18.75, 0.25)
JAN1_2021_JD = 2459215.5                                           # scanners' times before it are not trusted


def _policy_table(policies: Mapping) -> torch.Tensor:
    """[n_policies, 4] float64 on the host: thr, cut, k, gate (NaN = none)."""
    if len(policies) == 0:
        raise ValueError("policies is empty")
    rows = []
    for name, pol in policies.items():
        if len(pol) != 4:
            raise ValueError(f"policy {name!r} must be (thr, cut, k, gate), got {pol!r}")
        thr, cut, k, gate = pol
        rows.append([float(thr), float(cut), float(k), float("nan") if gate is None else float(gate)])
    return torch.tensor(rows, dtype=torch.float64)


def _policy_slots(object_id, jd, magpsf, label, raw_preds, policies: Mapping) -> Dict[str, torch.Tensor]:
    """The kernel over n object slots (objects in ascending id order first, then empty slots with n_alerts = 0), without
    a host synchronisation.  ``first`` is the index of each object's first alert in input order (n for an empty slot)."""
    cols = dict(jd=jd, magpsf=magpsf, label=label, raw_preds=raw_preds)
    for name, t in dict(object_id=object_id, **cols).items():
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a tensor, got {type(t).__name__}")
    n = _check_table("val.policy_eval", object_id, **cols)
    dev = object_id.device
    table = _policy_table(policies)
    npol = table.shape[0]
    jd, magpsf = (t.to(device=dev, dtype=torch.float64).contiguous() for t in (jd, magpsf))
    raw = raw_preds.to(device=dev, dtype=torch.float32).contiguous()
    lab = label.to(device=dev, dtype=torch.int32).contiguous()
    pred = torch.empty((n, npol), dtype=torch.int32, device=dev)               # the kernel writes every slot
    trig = torch.empty((n, npol, 2), dtype=torch.float64, device=dev)
    info = torch.empty((n, 3), dtype=torch.float64, device=dev)
    first = torch.zeros(n, dtype=torch.int64, device=dev)
    if n:
        perm, offsets = _group_by_object(object_id)
        first = torch.cat([perm.to(torch.int64), torch.full((1,), n, dtype=torch.int64, device=dev)])[offsets[:-1].long()]
        for p0 in range(0, npol, POLICIES_PER_LAUNCH):
            chunk = table[p0:p0 + POLICIES_PER_LAUNCH].contiguous()    # (a host array: it travels as kernel arguments)
            m = chunk.shape[0]
            whole = m == npol                      # one launch: write in place; a sweep: per-chunk buffers, copied in
            cp = pred if whole else torch.empty((n, m), dtype=torch.int32, device=dev)
            ct = trig if whole else torch.empty((n, m, 2), dtype=torch.float64, device=dev)
            _launch_grouped("btsbot_policy_eval", (perm, offsets), n, jd, magpsf, raw, lab,
                            C.cast(C.c_void_p(chunk.data_ptr()), C.POINTER(C.c_double)), m, cp, ct, info)
            if not whole:
                pred[:, p0:p0 + m] = cp
                trig[:, p0:p0 + m] = ct
    return {"first": first, "n_alerts": info[:, 0].to(torch.int64), "label": info[:, 1].to(torch.int64),
            "min_magpsf": info[:, 2], "pred": pred, "trigger_jd": trig[:, :, 0], "trigger_mag": trig[:, :, 1]}


def policy_eval(object_id: torch.Tensor, jd: torch.Tensor, magpsf: torch.Tensor, label: torch.Tensor,
                raw_preds: torch.Tensor, policies: Mapping = REFERENCE_POLICIES) -> Dict[str, torch.Tensor]:
    """Per object, on the inputs' device: does each policy fire, and at which alert first.

    object_id: any integers (equal = same object); jd, magpsf are taken as float64, raw_preds (the sigmoid scores) as
    float32 and compared as that value widened to float64, label as 0/1 integers.  policies: name -> (thr, cut, k,
    gate or None), in the order of the output's policy axis.  With P(i) the alerts of i's object up to and including i
    in (jd, input position) order, a policy fires at i when at least k alerts of P(i) have ``raw > thr and magpsf <
    cut`` and (without a gate, or) ``min magpsf over P(i) <= gate``; NaN magpsf are never valid and the minimum skips
    them.  jd must be finite (not checked).  Returns tensors over the objects, in ascending id order:

    ``object_id``; ``n_alerts``; ``label`` (of the object's first alert in input order); ``min_magpsf`` (NaN: none);
    ``first_alert`` (the input index of that first alert, to gather the caller's own per-object columns);
    ``pred`` int32 [n_obj, n_pol]; ``trigger_jd``, ``trigger_mag`` float64 [n_obj, n_pol]: the first alert the policy
    fires at, -1 when it never does.

    Grouping, the launches (one per 16 policies) and everything above run without a host synchronisation on n object
    slots; the number of objects is then read ONCE (one synchronisation, after all the work is queued) to cut the
    slots down to the objects."""
    slots = _policy_slots(object_id, jd, magpsf, label, raw_preds, policies)
    n_obj = int((slots["n_alerts"] > 0).sum().item()) if object_id.shape[0] else 0      # the one host read
    out = {k: v[:n_obj] for k, v in slots.items() if k != "first"}
    out["first_alert"] = slots["first"][:n_obj]
    out["object_id"] = object_id[out["first_alert"]]
    return out


def _median_columns(x: torch.Tensor) -> torch.Tensor:
    """np.nanmedian down every column of float64 [n, m]: the mean of the two middle values of an even count (which
    torch.nanmedian does not take, and which ``a + 0.5 * (b - a)`` of torch.nanquantile does not always round to);
    NaN for a column without a value."""
    n, m = x.shape
    if n == 0:
        return torch.full((m,), float("nan"), dtype=torch.float64, device=x.device)
    srt = torch.sort(x, dim=0).values                               # NaN sort last
    cnt = (~torch.isnan(x)).sum(0)
    lo = ((cnt - 1).clamp(min=0) // 2)[None]
    hi = (cnt // 2).clamp(max=n - 1)[None]
    med = (torch.gather(srt, 0, lo) + torch.gather(srt, 0, hi))[0] / 2
    return torch.where(cnt > 0, med, torch.full_like(med, float("nan")))


def policy_performance(object_id: torch.Tensor, jd: torch.Tensor, magpsf: torch.Tensor, label: torch.Tensor,
                       raw_preds: torch.Tensor, policies: Mapping = REFERENCE_POLICIES,
                       junk: Optional[torch.Tensor] = None, save_time: Optional[torch.Tensor] = None,
                       trigger_time: Optional[torch.Tensor] = None) -> dict:
    """The reference's ``policy_performance`` (val.py:425-614): ``{name: {policy_precision, policy_recall,
    binned_precision, binned_recall, peakmag_bins, med_save_dt, med_trigger_dt}}`` as Python floats and lists.

    The per-alert arguments are those of ``policy_eval``.  ``junk`` (bool), ``save_time`` and ``trigger_time`` (float64
    jd, NaN = not known) are per alert ROW, constant inside an object as a csv join yields them -- the object takes its
    first alert's -- or None (no junk; no time known).  An object is taken when it is not junk, has at least 2 alerts and
    is not (label 1 and min magpsf > 18.5).  Over the taken objects, per policy: TP / FP / FN / TN from (label, pred);
    the same counts over the ``np.histogram`` bins ``PEAKMAG_BINS`` of min magpsf (left-closed, 18.5 itself in the last
    bin, values outside dropped); precision = TP / (TP + FP), recall = TP / (TP + FN), per bin too (0 / 0 = NaN);
    ``med_save_dt`` = the median over TP objects with ``save_time >= 2459215.5`` and a trigger of ``trigger_jd -
    save_time``, ``med_trigger_dt`` the same with ``2459215.5 <= trigger_time < 1e10`` (nothing to take: NaN).  Without
    a TP or without a TN every figure is -999.0 and the binned lists are [-999.0], as there.

    Everything is reduced on the device over the kernel's object slots; ONE host read at the end."""
    names, rows, _ = _policy_performance_device(object_id, jd, magpsf, label, raw_preds, policies, junk, save_time,
                                                trigger_time)
    return _policy_performance_dict(names, rows.cpu().tolist())                           # the one host read


def _policy_performance_device(object_id, jd, magpsf, label, raw_preds, policies, junk, save_time, trigger_time):
    """``policy_performance`` up to its host read: the policy names, one float64 row of counts and medians per policy on
    the device, and per object slot and policy the ``save_dt`` that median is taken over (NaN where there is none; None
    without ``save_time``)."""
    columns = (("junk", junk, torch.bool), ("save_time", save_time, torch.float64),
               ("trigger_time", trigger_time, torch.float64))
    for name, t, _ in columns:                                        # before any device work
        if t is not None and (not isinstance(t, torch.Tensor) or t.dim() != 1 or t.shape[0] != len(object_id)):
            raise ValueError(f"{name} must be a tensor of [{len(object_id)}] alert rows")
    slots = _policy_slots(object_id, jd, magpsf, label, raw_preds, policies)
    dev, n = object_id.device, object_id.shape[0]
    names = list(policies)
    per_row = {}
    for name, t, dtype in columns:
        if t is None:
            continue
        pad = torch.zeros(1, dtype=dtype, device=dev) if dtype == torch.bool else \
            torch.full((1,), float("nan"), dtype=dtype, device=dev)
        per_row[name] = torch.cat([t.to(device=dev, dtype=dtype), pad])[slots["first"]]     # (empty slots: the pad)
    lab, peak, pred = slots["label"], slots["min_magpsf"].contiguous(), slots["pred"] == 1
    taken = (slots["n_alerts"] >= 2) & ~((lab == 1) & (peak > 18.5))
    if "junk" in per_row:
        taken &= ~per_row["junk"]
    pos, neg = (taken & (lab == 1))[:, None], (taken & (lab != 1))[:, None]
    tp, fp, fn, tn = pos & pred, neg & pred, pos & ~pred, neg & ~pred                     # [slots, n_pol]
    edges = torch.tensor(PEAKMAG_BINS, dtype=torch.float64, device=dev)
    nb = len(PEAKMAG_BINS) - 1
    which = (torch.bucketize(peak, edges, right=True) - 1).clamp(max=nb - 1)              # 18.5 itself: the last bin
    inside = (peak >= edges[0]) & (peak <= edges[-1])
    onehot = (which[:, None] == torch.arange(nb, device=dev)[None]) & inside[:, None]     # [slots, 6]
    counts = [m.sum(0).to(torch.float64)[:, None] for m in (tp, fp, fn, tn)]
    counts += [(m[:, :, None] & onehot[:, None, :]).sum(0).to(torch.float64) for m in (tp, fp, fn)]
    tjd = slots["trigger_jd"]
    meds, save_dt = [], None
    for t, upper in ((per_row.get("save_time"), None), (per_row.get("trigger_time"), 1e10)):
        if t is None:
            meds.append(torch.full((len(names), 1), float("nan"), dtype=torch.float64, device=dev))
            continue
        ok = t >= JAN1_2021_JD
        if upper is not None:
            ok &= t < upper
        dt = torch.where(tp & ok[:, None] & (tjd > 0), tjd - t[:, None], torch.full_like(tjd, float("nan")))
        if upper is None:
            save_dt = dt
        meds.append(_median_columns(dt)[:, None])
    return names, torch.cat(counts + meds, dim=1), save_dt


def _policy_performance_dict(names, rows) -> dict:
    nb = len(PEAKMAG_BINS) - 1
    nan = float("nan")
    out = {}
    for name, row in zip(names, rows):
        n_tp, n_fp, n_fn, n_tn = (int(v) for v in row[:4])
        btp, bfp, bfn = (row[4 + nb * j:4 + nb * (j + 1)] for j in range(3))
        if n_tp > 0 and n_tn > 0:
            out[name] = {"policy_precision": n_tp / (n_tp + n_fp), "policy_recall": n_tp / (n_tp + n_fn),
                         "binned_precision": [a / (a + b) if a + b > 0 else nan for a, b in zip(btp, bfp)],
                         "binned_recall": [a / (a + b) if a + b > 0 else nan for a, b in zip(btp, bfn)],
                         "peakmag_bins": list(PEAKMAG_BINS), "med_save_dt": row[-2], "med_trigger_dt": row[-1]}
        else:
            out[name] = {"policy_precision": -999.0, "policy_recall": -999.0, "binned_precision": [-999.0],
                         "binned_recall": [-999.0], "peakmag_bins": list(PEAKMAG_BINS), "med_save_dt": -999.0,
                         "med_trigger_dt": -999.0}
    return out
