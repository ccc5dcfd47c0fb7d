"""The overlap hint (btsbot_set_option "forwards_in_flight") and what it switches: stage2p on 7 alerts per workgroup and,
at 512 channels, the 1x1 stage (btsbot_amd/csrc/stage3.hip) on 64-alert fc1 / 64-channel fc2 tiles.

The tile shape changes which workgroup computes a value, not how: a row's LayerNorm, the k order of its fc1 sums, the
eight K slices of fc2 and `fmaf(g, b, s) + x` are the same in both shapes, so the logits are expected to be the same
bits.  Batches: a lone alert, a ragged 64-alert tile (33), one full tile (64), a tile plus one row (65), two tiles plus one
row (129).  stage2p is held at 5 alerts per workgroup on both sides, so the tiles are the only difference.

The option test talks to the C ABI only and needs no GPU (a handle's schedule is host state).
"""
import warnings

import pytest
import torch

import btsbot_amd
from helpers import CONFIGS, seeded_state, build_model, run_model
from btsbot_amd import _lib
from btsbot_amd.synthetic import synthetic_batch

BATCHES = (1, 33, 64, 65, 129)


def set_option(m, key, value):
    return _lib.lib().btsbot_set_option(m._handle.ptr, key, value)


@pytest.fixture(scope="module")
def case():
    kind, cfg = CONFIGS["mm_pico"]
    img, meta, _ = synthetic_batch(max(BATCHES), seed=11)
    return kind, cfg, seeded_state(kind, cfg, seed=3), img, meta


_models = {}


def model(case, cuda, prec):
    """one model per precision for the whole module (its handle exists from the first forward on)"""
    if prec not in _models:
        kind, cfg, sd, img, meta = case
        m = build_model(kind, cfg, sd, cuda, prec)
        run_model(kind, m, img[:1].to(cuda), meta[:1].to(cuda))
        _models[prec] = m
    return _models[prec]


def logits(case, cuda, m, n, in_flight):
    kind, _, _, img, meta = case
    _lib.check(set_option(m, b"stage2p_alerts", 5), "btsbot_set_option")
    _lib.check(set_option(m, b"forwards_in_flight", in_flight), "btsbot_set_option")
    try:
        assert m.schedule_flag("stage3") and m.schedule_flag("s3_wide") == bool(in_flight) and not m.schedule_flag("s2p_g7")
        return run_model(kind, m, img[:n].to(cuda), meta[:n].to(cuda)).cpu()
    finally:
        set_option(m, b"forwards_in_flight", 0)
        set_option(m, b"stage2p_alerts", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("n", BATCHES)
@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_wide_tiles_give_the_narrow_tiles_bits(cuda, case, prec, n):
    m = model(case, cuda, prec)
    narrow, wide = logits(case, cuda, m, n, 0), logits(case, cuda, m, n, 1)
    assert torch.isfinite(narrow).all() and narrow.shape[0] == n
    print(f"    {prec}, {n} alerts: max|wide - narrow| = {(wide - narrow).abs().max().item():.3e}")
    assert torch.equal(wide, narrow)


@pytest.mark.gpu
def test_fp8_wide_tiles_give_the_narrow_tiles_bits(cuda, case):
    """(fp8 takes the wide tiles under the hint too; the order of fc2's k inside a step is the packing's in both shapes)"""
    m = model(case, cuda, "fp8")
    narrow, wide = logits(case, cuda, m, 65, 0), logits(case, cuda, m, 65, 1)
    assert torch.isfinite(narrow).all() and torch.equal(wide, narrow)


@pytest.mark.gpu
def test_score_stream_equals_plain_calls(cuda, case):
    """depth 3, three batches of 65 alerts: every forward runs hinted (7 alerts per stage-2 workgroup, wide tiles) on a
    replica of its own; a plain call runs the default schedule"""
    kind, cfg, sd, img, meta = case
    m = model(case, cuda, "bf16")
    batches = [(img[i:i + 65].to(cuda), meta[i:i + 65].to(cuda)) for i in (0, 32, 64)]
    plain = [run_model(kind, m, *b).cpu() for b in batches]
    assert not m.schedule_flag("s3_wide") and not m.schedule_flag("s2p_g7")
    scorer = btsbot_amd.ScoreStream(m, depth=3)
    tickets = [scorer.submit(*b) for b in batches]
    got = [scorer.result(t).cpu() for t in tickets]
    for twin in scorer.models:   # the hint is taken back behind each forward
        assert not twin.schedule_flag("s3_wide") and not twin.schedule_flag("s2p_g7")
    for a, b in zip(got, plain):
        assert torch.equal(a, b)


def host_model(name, prec):
    kind, cfg = CONFIGS[name]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return getattr(btsbot_amd, kind)(cfg, precision=prec)


def flags(m):
    return m.schedule_flag("s3_wide"), m.schedule_flag("s2p_g7")


def test_forwards_in_flight_option(monkeypatch):
    monkeypatch.delenv("BTSBOT_AMD_S3_TILES", raising=False)
    monkeypatch.delenv("BTSBOT_AMD_S2P_G", raising=False)
    for prec in ("bf16", "f16", "fp8"):
        m = host_model("mm_pico", prec)
        assert flags(m) == (False, False), prec
        assert set_option(m, b"forwards_in_flight", 1) == _lib.OK
        assert flags(m) == (True, True), prec
        assert set_option(m, b"forwards_in_flight", 0) == _lib.OK
        assert flags(m) == (False, False), prec
        # the caller's alerts per workgroup win over the hint, in either order; the tiles are the hint's alone
        assert set_option(m, b"stage2p_alerts", 5) == _lib.OK and set_option(m, b"forwards_in_flight", 1) == _lib.OK
        assert flags(m) == (True, False), prec
        assert set_option(m, b"stage2p_alerts", 0) == _lib.OK
        assert flags(m) == (True, True), prec
        assert set_option(m, b"forwards_in_flight", 0) == _lib.OK and set_option(m, b"stage2p_alerts", 7) == _lib.OK
        assert flags(m) == (False, True), prec
        assert set_option(m, b"forwards_in_flight", 2) == _lib.ERR_INVALID_ARG
        assert b"forwards_in_flight" in _lib.lib().btsbot_last_error()
        assert flags(m) == (False, True), prec
    # handles without wide tiles take the option and keep their tiles: fp32 runs no stage3.hip, split fragments are 8 registers
    for prec in ("f32", "f16x2"):
        m = host_model("mm_pico", prec)
        assert set_option(m, b"forwards_in_flight", 1) == _lib.OK
        assert not m.schedule_flag("s3_wide"), prec
        assert not m.schedule_flag("s2p_g7"), prec          # (f16x2: stage2p's split planes hold 5 alerts at most)
        assert set_option(m, b"forwards_in_flight", 0) == _lib.OK
    assert m.schedule_flag("stage3")                        # (f16x2 does run stage3.hip, on narrow tiles)
    # no image branch: nothing to decide, still accepted
    m = host_model("um_nn", "bf16")
    assert set_option(m, b"forwards_in_flight", 1) == _lib.OK and flags(m) == (False, False)
    # 640 channels (nano): wide tiles with or without the hint, as before
    m = host_model("mm_nano_ls", "bf16")
    assert flags(m) == (True, False)
    assert set_option(m, b"forwards_in_flight", 1) == _lib.OK and flags(m) == (True, True)
