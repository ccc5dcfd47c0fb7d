"""CPU-side checks of the embedding outputs (btsbot_embed_width / model.embedding_dim / model.embed / ScoreStream(embed=)):
widths per wiring, argument errors and the refusals that need no GPU.  No compute call is made."""
import warnings

import pytest
import torch

import btsbot_amd
from btsbot_amd import _lib
from helpers import CONFIGS, MV_CONFIGS

_ALL = dict(CONFIGS, **MV_CONFIGS)


def _model(name, **kw):
    kind, cfg = _ALL[name]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return getattr(btsbot_amd, kind)(cfg, **kw)


def _expected_widths(name):
    """(features, hidden) from the config alone: image width of the backbone + meta_fc2 of whichever branch exists;
    comb_fc2 / fc2_neurons, and for um_nn the features again."""
    kind, cfg = _ALL[name]
    icfg = cfg.get("image_model_config", cfg)
    mcfg = cfg.get("meta_model_config", cfg)
    img = 0
    if kind != "um_nn":
        img = 640 if "nano" in icfg["model_kind"] else 512          # convnext_pico and maxvit_tiny_rw_224: 512
    meta = mcfg["meta_fc2_neurons"] if kind not in ("ConvNeXt", "MaxViT") else 0
    features = img + meta
    hidden = features if kind == "um_nn" else cfg.get("comb_fc2_neurons", cfg.get("fc2_neurons"))
    return features, hidden


@pytest.mark.parametrize("name", list(_ALL))
def test_embedding_widths_per_wiring(name):
    m = _model(name)
    features, hidden = _expected_widths(name)
    L = _lib.lib()
    assert L.btsbot_embed_width(m._handle.ptr, 0) == features
    assert L.btsbot_embed_width(m._handle.ptr, 1) == hidden
    assert m.embedding_dim("features") == features and m.embedding_dim("hidden") == hidden
    assert m.embedding_dim() == features
    for prec in ("bf16", "f16x2"):                                   # the width is the wiring's, not the mode's
        m.set_precision(prec)
        assert (m.embedding_dim("features"), m.embedding_dim("hidden")) == (features, hidden)


def test_table_of_widths_is_what_the_issue_lists():
    got = {n: _expected_widths(n) for n in _ALL}
    assert got == {"mm_pico": (640, 32), "mm_nano_ls": (768, 32), "convnext": (512, 16), "um_nn": (64, 64),
                   "frozen_fusion": (576, 16), "mm_maxvit": (640, 32), "maxvit": (512, 16),
                   "frozen_fusion_maxvit": (576, 16)}


def test_embed_width_rejects_an_unknown_embedding():
    m = _model("mm_pico")
    L = _lib.lib()
    for which in (-1, 2, 99):
        assert L.btsbot_embed_width(m._handle.ptr, which) == _lib.ERR_INVALID_ARG
        assert b"embed_width" in L.btsbot_last_error()
    assert L.btsbot_embed_width(None, 0) == _lib.ERR_INVALID_ARG
    with pytest.raises(ValueError):
        m.embedding_dim("logits")


def test_embed_has_no_cpu_fallback():
    m = _model("mm_pico").eval()
    img, meta = torch.zeros(2, 3, 63, 63), torch.zeros(2, 25)
    with pytest.raises(RuntimeError, match="no CPU fallback") as fwd:
        m(image_input=img, metadata_input=meta)
    with pytest.raises(RuntimeError, match="no CPU fallback") as emb:
        m.embed(image_input=img, metadata_input=meta)
    assert str(emb.value) == str(fwd.value)
    u = _model("um_nn").eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        u.embed(input_data=meta, layer="hidden", return_logits=True)


def test_embed_argument_errors():
    m = _model("mm_pico")
    img, meta = torch.zeros(2, 3, 63, 63), torch.zeros(2, 25)
    assert m.training
    with pytest.raises(RuntimeError, match="eval mode"):             # train mode: before any device check
        m.embed(image_input=img, metadata_input=meta)
    m.eval()
    with pytest.raises(ValueError, match="unknown embedding layer"):
        m.embed(image_input=img, metadata_input=meta, layer="logits")
    with pytest.raises(ValueError, match="unknown embedding layer"):
        m.train().embed(image_input=img, metadata_input=meta, layer="logits")   # the layer is checked first
    m.eval()
    with pytest.raises(TypeError):                                   # forward's own keywords, nothing else
        m.embed(input_data=img)
    with pytest.raises(TypeError):
        m.embed(img)
    with pytest.raises(ValueError):                                  # forward's own shape checks
        m.embed(image_input=img[:, :, :60, :60], metadata_input=meta)


def test_score_stream_rejects_an_unknown_embed_value():
    m = _model("um_nn").eval()
    with pytest.raises(ValueError, match="embed must be"):
        btsbot_amd.ScoreStream(m, depth=1, embed="logits")
    with pytest.raises(RuntimeError, match="no CPU fallback"):       # a known value gets as far as the device check
        btsbot_amd.ScoreStream(m, depth=1, embed="features")


def test_run_training_no_longer_ignores_generate_embeddings():
    import inspect
    from btsbot_amd import train
    assert "generate_embeddings" in inspect.getsource(train.run_training)
    assert callable(train.write_embeddings)
