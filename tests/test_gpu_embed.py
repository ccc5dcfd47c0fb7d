"""GPU tests of the embedding outputs (run with -m gpu on an MI355X): model.embed / btsbot_forward_embed /
ScoreStream(embed=) / run_training's generate_embeddings step against the fp32 CPU oracle and against themselves.

`features` is the input row of the first fusion / head Linear, `hidden` the input row of the last Linear
(include/btsbot_hip.h).  The oracle side is composed here from the oracle's public functions, unmodified.

Bound on the distance from the oracle, in the form the logits already use (tests/test_gpu_parity.py):
    max|d| <= T[prec] * max(1, max|ref|)          per layer, over all alerts and columns.
T is twice the worst value measured on the GPU over the wirings below x both layers x three weight seeds (3, 11, 12;
39 alerts for the ConvNeXt wirings, 8 for the MaxViT ones), per precision:
    precision   measured worst     T
    f32         2.647e-06        5.294e-06
    f16x2       1.125e-05        2.250e-05
    f16         1.988e-03        3.976e-03
    bf16        1.665e-02        3.330e-02
    fp8         4.365e-03        8.730e-03      (mm_pico only)
T["f32"] may not exceed the logits' own 1e-4 (TOL_LOGIT_REL["f32"]).
"""
import ctypes as C
import os
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import CONFIGS, MV_CONFIGS, seeded_state, seeded_state_mv, build_model, run_model
from btsbot_amd import _lib
from btsbot_amd.synthetic import synthetic_batch
from oracle import convnext_oracle as O   # checker only

pytestmark = pytest.mark.gpu

T = {"f32": 5.294e-6, "f16x2": 2.25e-5, "f16": 3.976e-3, "bf16": 3.33e-2, "fp8": 8.73e-3}
TOL_LOGIT_F32 = 1e-4                    # tests/test_gpu_parity.py: TOL_LOGIT_REL["f32"]
assert T["f32"] <= TOL_LOGIT_F32

# how each wiring is put together: (image prefix, head LayerNorm?, metadata prefix, metadata trailing activation,
#  the three head Linears, activation)
_COMB = ("combined_head.0.", "combined_head.2.", "combined_head.5.")
_WIRING = {
    "mm_ConvNeXt": ("convnext_backbone.", None, "metadata_branch.", True, _COMB, "gelu"),
    "ConvNeXt": ("convnext.", True, None, None, ("convnext.head.3.", "convnext.head.5.", "convnext.head.8."), "gelu"),
    "um_nn": (None, None, "network.", True, ("network.6.",), "relu"),
    "frozen_fusion": ("image_branch.convnext.", True, "meta_branch.network.", False, _COMB, "relu"),
    "mm_MaxViT": ("maxvit_backbone.", None, "metadata_branch.", True, _COMB, "gelu"),
    "MaxViT": ("maxvit.", None, None, None, ("maxvit.head.1.", "maxvit.head.3.", "maxvit.head.6."), "gelu"),
    "frozen_fusion_MaxViT": ("image_branch.maxvit.", None, "meta_branch.network.", False, _COMB, "relu"),
}


def _wiring(kind, cfg):
    if kind == "frozen_fusion" and cfg["image_model_config"]["model_name"] == "MaxViT":
        return _WIRING["frozen_fusion_MaxViT"]
    w = _WIRING[kind]
    if kind == "mm_ConvNeXt":
        return (w[0], "LS" in cfg["train_data_version"]) + w[2:]
    return w


def _head(sd, keys, act, x):
    """(hidden, logits) of the head's Linears on `x` -- fusion_head itself where the head has its three layers."""
    if len(keys) == 1:
        return x, F.linear(x, sd[keys[0] + "weight"], sd[keys[0] + "bias"])
    view = {f"h.{n}.{leaf}": sd[k + leaf] for n, k in zip((0, 2, 5), keys) for leaf in ("weight", "bias")}
    a = F.gelu if act == "gelu" else F.relu
    hidden = a(F.linear(a(F.linear(x, view["h.0.weight"], view["h.0.bias"])), view["h.2.weight"], view["h.2.bias"]))
    return hidden, O.fusion_head(x, view, "h.", act)


def oracle_embeddings(kind, cfg, sd, img, meta):
    """(features, hidden, logits) of the fp32 CPU oracle."""
    ip, norm, mp, trailing, keys, act = _wiring(kind, cfg)
    parts = []
    with torch.no_grad():
        if ip is not None:
            icfg = cfg.get("image_model_config", cfg)
            if "maxvit" in ip:
                from oracle import maxvit_oracle as MO
                arch = MO.arch_of(icfg.get("model_kind", "maxvit_tiny_rw_224.sw_in1k"))
                parts.append(MO.pooled(MO.forward_features(MO.resize(img, MO.ARCHS[arch]["img"]), sd, ip, arch)))
            else:
                x = O.forward_features(img, sd, ip, O.arch_of(icfg.get("model_kind", "convnext_nano.d1h_in1k")))
                parts.append(O.pooled_head(x, sd[ip + "head.1.weight"] if norm else None,
                                           sd[ip + "head.1.bias"] if norm else None))
        if mp is not None:
            parts.append(O.metadata_branch(meta, sd, mp, act, trailing))
        features = torch.cat(parts, dim=1)
        hidden, logits = _head(sd, keys, act, features)
    return features, hidden, logits


def _inputs(kind, img, meta):
    if kind in ("mm_ConvNeXt", "frozen_fusion", "mm_MaxViT"):
        return dict(image_input=img, metadata_input=meta)
    return dict(input_data=img if kind in ("ConvNeXt", "MaxViT") else meta)


def gpu_embeddings(kind, m, img, meta):
    """(features, hidden, logits) of the model under test, on the CPU."""
    kw = _inputs(kind, img, meta)
    features, logits = m.embed(layer="features", return_logits=True, **kw)
    hidden = m.embed(layer="hidden", **kw)
    return features.cpu(), hidden.cpu(), logits.cpu()


def rel_dev(got, ref):
    return (got - ref).abs().max().item() / max(1.0, ref.abs().max().item())


def _consistent(kind, cfg, sd, features, hidden, logits):
    """The returned rows reproduce the returned logits through the oracle's own head, on the CPU: a wrong slice, order
    or activation fails here whatever the backbone's tolerance (the heads are fp32-class in every mode)."""
    _ip, _norm, _mp, _tr, keys, act = _wiring(kind, cfg)
    with torch.no_grad():
        _h, from_features = _head(sd, keys, act, features)
        from_hidden = F.linear(hidden, sd[keys[-1] + "weight"], sd[keys[-1] + "bias"])
    scale = max(1.0, logits.abs().max().item())
    d1, d2 = (from_features - logits).abs().max().item(), (from_hidden - logits).abs().max().item()
    print(f"   self-consistency: head(features) {d1 / scale:.3e}, last(hidden) {d2 / scale:.3e} (bound {TOL_LOGIT_F32})")
    assert d1 <= TOL_LOGIT_F32 * scale, f"fusion_head(features) vs logits: {d1} (scale {scale})"
    assert d2 <= TOL_LOGIT_F32 * scale, f"last Linear(hidden) vs logits: {d2} (scale {scale})"


def _parity_case(cuda, kind, cfg, sd, n_alerts, prec):
    img, meta, _ = synthetic_batch(n_alerts, seed=2)
    rf, rh, _rl = oracle_embeddings(kind, cfg, sd, img, meta)
    m = build_model(kind, cfg, sd, cuda, prec)
    assert (m.embedding_dim("features"), m.embedding_dim("hidden")) == (rf.shape[1], rh.shape[1])
    f, h, z = gpu_embeddings(kind, m, img.to(cuda), meta.to(cuda))
    for name, got, ref in (("features", f, rf), ("hidden", h, rh)):
        assert got.shape == ref.shape and got.dtype == torch.float32 and got.is_contiguous()
        assert torch.isfinite(got).all()
        dev = rel_dev(got, ref)
        print(f"   {kind} {prec} {name}: max|d| / max(1, max|ref|) = {dev:.3e} (bound {T[prec]:.1e})")
        assert dev <= T[prec], f"{prec} {name}: {dev}"
    _consistent(kind, cfg, sd, f, h, z)


_CN_CASES = [(n, p) for n in CONFIGS for p in ("f32", "f16x2", "f16", "bf16")] + [("mm_pico", "fp8")]


@pytest.mark.parametrize("name,prec", _CN_CASES, ids=[f"{n}-{p}" for n, p in _CN_CASES])
def test_embeddings_match_oracle(cuda, name, prec):
    kind, cfg = CONFIGS[name]
    _parity_case(cuda, kind, cfg, seeded_state(kind, cfg, seed=3), 39, prec)


@pytest.mark.parametrize("name", list(MV_CONFIGS))
@pytest.mark.parametrize("prec", ["f32", "f16x2"])
def test_maxvit_embeddings_match_oracle(cuda, name, prec):
    kind, cfg = MV_CONFIGS[name]
    _parity_case(cuda, kind, cfg, seeded_state_mv(kind, cfg, seed=3), 8, prec)


def test_branch_identity(cuda):
    """What frozen_fusion is built on: the image half of its features is the ConvNeXt model's features, and its metadata
    half is the um_nn model's features in front of their ReLU (the reference strips that activation with the head)."""
    kind, cfg = CONFIGS["frozen_fusion"]
    sd = seeded_state(kind, cfg, seed=5)
    ikind, icfg = CONFIGS["convnext"]
    mkind, mcfg = CONFIGS["um_nn"]
    assert cfg["image_model_config"] == icfg and cfg["meta_model_config"] == mcfg
    isd, msd = seeded_state(ikind, icfg, seed=6), seeded_state(mkind, mcfg, seed=7)
    n_img = n_meta = 0
    for k, v in sd.items():
        if k.startswith("image_branch."):
            isd[k[len("image_branch."):]] = v
            n_img += 1
        elif k.startswith("meta_branch."):
            msd[k[len("meta_branch."):]] = v
            n_meta += 1
    assert n_img == len(isd) - 6 and n_meta == len(msd) - 2        # all but the branch models' own heads
    img, meta, _ = synthetic_batch(21, seed=8)
    img, meta = img.to(cuda), meta.to(cuda)
    fus = build_model(kind, cfg, sd, cuda, "f32").embed(image_input=img, metadata_input=meta)
    d3 = 512
    image_only = build_model(ikind, icfg, isd, cuda, "f32").embed(input_data=img)
    meta_only = build_model(mkind, mcfg, msd, cuda, "f32").embed(input_data=meta)
    assert fus.shape == (21, d3 + 64) and image_only.shape == (21, d3) and meta_only.shape == (21, 64)
    assert rel_dev(fus[:, :d3].cpu(), image_only.cpu()) <= T["f32"]
    assert rel_dev(torch.relu(fus[:, d3:]).cpu(), meta_only.cpu()) <= T["f32"]
    assert (fus[:, d3:] < 0).any()                                   # the fusion's half really is pre-activation


def _abi_embed(m, img, meta, B, rows, with_embeddings=True):
    """btsbot_forward_embed through the binding on buffers of `rows` rows pre-filled with NaN."""
    dev = (img if img is not None else meta).device
    wf, wh = m.embedding_dim("features"), m.embedding_dim("hidden")
    logits = torch.full((rows,), float("nan"), device=dev)
    feats = torch.full((rows, wf), float("nan"), device=dev)
    hid = torch.full((rows, wh), float("nan"), device=dev)
    with torch.cuda.device(dev):
        L, stream = m._prepare(dev, B)
        _lib.check(L.btsbot_forward_embed(
            m._handle.ptr, C.c_void_p(img.data_ptr() if img is not None else 0),
            C.c_void_p(meta.data_ptr() if meta is not None else 0), C.c_void_p(logits.data_ptr()), C.c_void_p(0),
            C.c_void_p(feats.data_ptr() if with_embeddings else 0), C.c_void_p(hid.data_ptr() if with_embeddings else 0),
            B, C.c_void_p(stream)), "btsbot_forward_embed")
    torch.cuda.synchronize()
    return logits, feats, hid


_TAIL_CASES = [("mm_pico", "f32"), ("mm_pico", "bf16"), ("um_nn", "bf16"), ("convnext", "f16")]


@pytest.mark.parametrize("name,prec", _TAIL_CASES, ids=[f"{n}-{p}" for n, p in _TAIL_CASES])
def test_tails_and_chunks(cuda, name, prec):
    """Batches that end inside a head workgroup (8 alerts in the fp32 head, 16 in the matrix-pipe head) and one that
    spans internal chunks (a chunk limit of 32 alerts: 77 = 32 + 32 + 13), through the C ABI with both embedding
    pointers set, on buffers 8 rows longer than the batch: rows < B equal a single-chunk run, rows >= B are untouched.
    The single-chunk run is model.embed on the batch's own chunks, one call each (an alert's position in its chunk is
    then the same in both runs: the 16-bit stage kernels' summation order depends on it, the heads' does not)."""
    kind, cfg = CONFIGS[name]
    sd = seeded_state(kind, cfg, seed=3)
    img, meta, _ = synthetic_batch(77, seed=9)
    img = img.to(cuda) if kind != "um_nn" else None
    meta = meta.to(cuda) if kind != "ConvNeXt" else None
    ref_model = build_model(kind, cfg, sd, cuda, prec)
    m = build_model(kind, cfg, sd, cuda, prec)
    m._max_chunk = 32
    for B in (1, 7, 8, 39, 77):
        a = img[:B].contiguous() if img is not None else None
        b = meta[:B].contiguous() if meta is not None else None
        logits, feats, hid = _abi_embed(m, a, b, B, B + 8)
        want_f, want_h, want_z = [], [], []
        for c0 in range(0, B, 32):
            kw = _inputs(kind, a[c0:c0 + 32] if a is not None else None, b[c0:c0 + 32] if b is not None else None)
            f, z = ref_model.embed(layer="features", return_logits=True, **kw)
            want_f.append(f), want_z.append(z.reshape(-1)), want_h.append(ref_model.embed(layer="hidden", **kw))
        for got, want in ((logits, torch.cat(want_z)), (feats, torch.cat(want_f)), (hid, torch.cat(want_h))):
            assert torch.isfinite(got[:B]).all(), (B, "rows < B")
            assert torch.equal(got[:B], want), (B, (got[:B] - want).abs().max().item())
            assert torch.isnan(got[B:]).all(), (B, "rows >= B were written")


def test_chunked_f32_equals_one_chunk(cuda):
    """The f32 mode's arithmetic does not depend on an alert's position: 77 alerts in chunks of 32 equal the same 77 in one
    chunk, bit for bit, in both rows and the logits (per-chunk offsets b0 * width)."""
    kind, cfg = CONFIGS["mm_pico"]
    sd = seeded_state(kind, cfg, seed=3)
    img, meta, _ = synthetic_batch(77, seed=9)
    img, meta = img.to(cuda), meta.to(cuda)
    whole = build_model(kind, cfg, sd, cuda, "f32")
    chunked = build_model(kind, cfg, sd, cuda, "f32")
    chunked._max_chunk = 32
    for layer in ("features", "hidden"):
        e1, z1 = whole.embed(image_input=img, metadata_input=meta, layer=layer, return_logits=True)
        e2, z2 = chunked.embed(image_input=img, metadata_input=meta, layer=layer, return_logits=True)
        assert torch.equal(e1, e2) and torch.equal(z1, z2)


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_scoring_is_unchanged(cuda, prec):
    kind, cfg = CONFIGS["mm_pico"]
    sd = seeded_state(kind, cfg, seed=3)
    img, meta, _ = synthetic_batch(39, seed=2)
    img, meta = img.to(cuda), meta.to(cuda)
    m = build_model(kind, cfg, sd, cuda, prec)
    plain = run_model(kind, m, img, meta).clone()
    for layer in ("features", "hidden"):
        _e, z = m.embed(image_input=img, metadata_input=meta, layer=layer, return_logits=True)
        assert z.shape == (39, 1) and torch.equal(z, plain)
    z_null, feats, hid = _abi_embed(m, img, meta, 39, 39, with_embeddings=False)
    assert torch.equal(z_null.view(39, 1), plain)
    assert torch.isnan(feats).all() and torch.isnan(hid).all()
    assert torch.equal(run_model(kind, m, img, meta), plain)         # and a scoring call afterwards


def test_embed_of_an_empty_batch(cuda):
    kind, cfg = CONFIGS["mm_pico"]
    m = build_model(kind, cfg, seeded_state(kind, cfg, seed=3), cuda, "bf16")
    e, z = m.embed(image_input=torch.zeros(0, 3, 63, 63, device=cuda), metadata_input=torch.zeros(0, 25, device=cuda),
                   return_logits=True)
    assert e.shape == (0, 640) and z.shape == (0, 1) and e.dtype == torch.float32
    assert m.embed(image_input=torch.zeros(0, 3, 63, 63, device=cuda), metadata_input=torch.zeros(0, 25, device=cuda),
                   layer="hidden").shape == (0, 32)


def test_score_stream_with_embeddings(cuda):
    import btsbot_amd
    kind, cfg = CONFIGS["mm_pico"]
    m = build_model(kind, cfg, seeded_state(kind, cfg, seed=3), cuda, "bf16")
    batches = []
    for i, n in enumerate((33, 64, 7, 128, 1)):
        img, meta, _ = synthetic_batch(n, seed=20 + i)
        batches.append((img.to(cuda), meta.to(cuda)))
    ref = [m.embed(image_input=a, metadata_input=b, return_logits=True) for a, b in batches]
    scorer = btsbot_amd.ScoreStream(m, depth=3, embed="features")
    for _ in range(2):
        outs = list(scorer.map(batches))
        torch.cuda.synchronize()
        assert len(outs) == len(ref)
        for (z, e), (re, rz) in zip(outs, ref):
            assert z.shape == rz.shape and e.shape == re.shape
            assert torch.equal(z, rz) and torch.equal(e, re)
    # the default is untouched: plain logits
    out = list(btsbot_amd.ScoreStream(m, depth=2).map(batches[:2]))
    assert all(isinstance(o, torch.Tensor) and torch.equal(o, r[1]) for o, r in zip(out, ref))


@pytest.mark.parametrize("with_test_split", [True, False])
def test_run_training_writes_embeddings(cuda, tmp_path, with_test_split):
    """config['generate_embeddings']: the rows of embeddings/<model>_<run>.npy are model.embed of the saved best checkpoint
    on the test split (with its candid column next to them), on the validation split when there are no test files."""
    import pandas as pd
    import btsbot_amd
    from btsbot_amd.train import run_training
    from helpers import METADATA_COLS
    _, meta, _ = synthetic_batch(448, seed=21)
    lab = (meta[:, 5] > meta[:, 5].median()).long().numpy()
    d = tmp_path / "data"
    d.mkdir()
    splits = [("train", slice(0, 256)), ("val", slice(256, 384))] + ([("test", slice(384, 448))] if with_test_split else [])
    for split, sl in splits:
        df = pd.DataFrame(meta[sl].numpy(), columns=METADATA_COLS)
        df["label"] = lab[sl]
        if split == "test":
            df["candid"] = np.arange(sl.start, sl.stop) + 1_000_000
        df.to_csv(d / f"{split}_cand_v11_N100.csv", index=False)
    cfg = dict(CONFIGS["um_nn"][1], model_name="um_nn", train_data_version="v11", epochs=2, batch_size=64,
               learning_rate="3e-3", warmup_epochs=1, beta_1=0.9, beta_2=0.999, patience=3, random_seed=2,
               generate_embeddings=True)
    hist, model_dir = run_training(cfg, data_base_dir=str(tmp_path) + "/", run_name="e0", device=cuda, precision="f32",
                                   models_root=str(tmp_path / "models"), embeddings_root=str(tmp_path / "embeddings"))
    path = tmp_path / "embeddings" / "um_nn_e0.npy"
    assert os.path.isfile(path) and hist["embeddings_file"] == str(path)
    got = np.load(path)
    sl = splits[-1][1]
    assert got.dtype == np.float32 and got.shape == (sl.stop - sl.start, 64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        best = btsbot_amd.um_nn(cfg, precision="f32")
    best.load_state_dict(torch.load(model_dir + "best_model.pth"), strict=True)
    want = best.to(cuda).eval().embed(input_data=meta[sl].to(cuda)).cpu().numpy()
    assert np.array_equal(got, want)
    csv = tmp_path / "embeddings" / "um_nn_e0.csv"
    if with_test_split:
        assert list(pd.read_csv(csv)["candid"]) == list(np.arange(sl.start, sl.stop) + 1_000_000)
    else:
        assert not os.path.exists(csv)
    # a run without the key writes nothing
    cfg2 = dict(cfg, generate_embeddings=False)
    run_training(cfg2, data_base_dir=str(tmp_path) + "/", run_name="e1", device=cuda, precision="f32",
                 models_root=str(tmp_path / "models"), embeddings_root=str(tmp_path / "embeddings"))
    assert not os.path.exists(tmp_path / "embeddings" / "um_nn_e1.npy")
