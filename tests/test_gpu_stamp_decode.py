"""btsbot_decode_stamps on the device: the corpus of tests/test_stamp_decode_host.py (its writer, its zlib / decode_stamp
oracles) through decode_stamps_device and make_triplets(decode="device").

No host synchronisation under fallback=None, by inspection (tests/test_gpu_feature_state.py has no run-time check to
copy): decode_stamps_device builds the offsets and the joined bytes in one host buffer, uploads it with one .to(device),
allocates its outputs and workspace with torch.empty and queues one launch; make_triplets(fallback=None) then calls
prep_triplets (one launch) and ORs the drop flags with (status != 0).any(1) on the device.  There is no .item(), .cpu(),
.tolist(), nonzero or bool() of a device tensor on that path -- the one host read, status.cpu(), sits behind
`if fallback == "host"`.  test_fallback_none_reads_nothing_back pins that down on the source."""
import inspect
import zlib

import numpy as np
import pytest
import torch

from btsbot_amd import alert_utils
from test_stamp_decode_host import (OK, UNSUPPORTED, deferred_corpus, frame_of, malformed_corpus, same_bits, stamp,
                                    valid_corpus, _images)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def corpus():
    """(stamps, expected frames [n,63,63], shapes [n,2], statuses [n]): the valid corpus with the deferred cases
    interleaved, decoded once on the host."""
    valid, deferred = valid_corpus(), deferred_corpus()
    stamps, frames, shapes, status = [], [], [], []
    for k, (_, s) in enumerate(valid):
        img = alert_utils.decode_stamp(s)
        stamps.append(s)
        frames.append(frame_of(img))
        shapes.append(img.shape)
        status.append(OK)
        if k % 7 == 3 and deferred:
            stamps.append(deferred.pop(0)[1])
            frames.append(np.zeros((63, 63), np.float32))
            shapes.append((0, 0))
            status.append(UNSUPPORTED)
    assert not deferred
    return stamps, np.stack(frames), np.array(shapes, dtype=np.int32), np.array(status, dtype=np.uint8)


def _decode(stamps, cuda):
    raw, shapes, status = alert_utils.decode_stamps_device(stamps, cuda)
    assert raw.dtype == torch.float32 and shapes.dtype == torch.int32 and status.dtype == torch.uint8
    assert raw.shape == (len(stamps), 63, 63) and shapes.shape == (len(stamps), 2) and status.shape == (len(stamps),)
    return raw.cpu().numpy(), shapes.cpu().numpy(), status.cpu().numpy()


def _check(got, stamps_idx, corpus):
    _, frames, shapes, status = corpus
    raw, shp, st = got
    assert np.array_equal(st, status[stamps_idx]), (st, status[stamps_idx])
    assert np.array_equal(shp, shapes[stamps_idx])
    for k, i in enumerate(stamps_idx):
        assert same_bits(raw[k], frames[i]), (k, i)
        h, w = shp[k]
        assert not raw[k, h:, :].view(np.uint32).any() and not raw[k, :, w:].view(np.uint32).any(), (k, i)


def test_valid_corpus_and_deferred_cases_in_one_call(cuda, corpus):
    stamps, _, _, status = corpus
    assert (status == OK).sum() == 33 and (status == UNSUPPORTED).sum() == 5      # nothing valid is deferred
    _check(_decode(stamps, cuda), np.arange(len(stamps)), corpus)


@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, 130])
def test_batch_sizes(cuda, corpus, n):
    """Neighbouring stamps of very different compressed lengths (the constant image is ~100 bytes, a stored noise
    image 23 kB): a seeded draw over the corpus that starts with the two extremes."""
    stamps = corpus[0]
    by_len = np.argsort([len(s) for s in stamps])
    idx = np.concatenate([[by_len[0], by_len[-1], by_len[1]], np.random.default_rng(n).integers(0, len(stamps), 130)])[:n]
    _check(_decode([stamps[i] for i in idx], cuda), idx, corpus)


def test_blob_at_an_odd_offset_of_a_larger_tensor(cuda, corpus):
    import ctypes as C
    from btsbot_amd import _lib
    stamps = corpus[0]
    idx = np.array([0, 5, 9, 2, 30])
    lens = [len(stamps[i]) for i in idx]
    blob = torch.frombuffer(bytearray(b"\xff" * 7 + b"".join(stamps[i] for i in idx) + b"\xff" * 9), dtype=torch.uint8).to(cuda)
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int64, device=cuda)
    n = len(idx)
    raw = torch.full((n, 63, 63), 5.0, device=cuda)
    shapes = torch.full((n, 2), -1, dtype=torch.int32, device=cuda)
    status = torch.full((n,), 99, dtype=torch.uint8, device=cuda)
    L = _lib.lib()
    ws_bytes = L.btsbot_decode_stamps_workspace(n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=cuda)
    assert (blob.data_ptr() + 7) % 2 == 1
    _lib.check(L.btsbot_decode_stamps(C.c_void_p(blob.data_ptr() + 7), C.c_void_p(offsets.data_ptr()), n,
                                      C.c_void_p(raw.data_ptr()), C.c_void_p(shapes.data_ptr()),
                                      C.c_void_p(status.data_ptr()), C.c_void_p(ws.data_ptr()), ws_bytes,
                                      C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)), "btsbot_decode_stamps")
    _check((raw.cpu().numpy(), shapes.cpu().numpy(), status.cpu().numpy()), idx, corpus)


def test_more_stamps_than_workspace_slots(cuda):
    """The workspace stops growing at 32,768 stamps in flight; past that the waves walk the batch.  32,838 small stamps
    of five kinds (one of them deferred), compared on the device."""
    from btsbot_amd import _lib
    noise = _images()[0]
    kinds = [stamp(noise[:1, :1]), stamp(noise[:3, :5]), stamp(noise[:2, :63], dict(level=0)),
             dict(deferred_corpus())["bitpix16_scaled"], stamp(noise[:7, :2], dict(strategy=zlib.Z_RLE))]
    n = 32768 + 70
    assert _lib.lib().btsbot_decode_stamps_workspace(n) == 32768 * 28800
    idx = np.random.default_rng(3).integers(0, len(kinds), n)
    raw, shapes, status = alert_utils.decode_stamps_device([kinds[i] for i in idx], cuda)
    frames = np.stack([np.zeros((63, 63), np.float32) if k == 3 else frame_of(alert_utils.decode_stamp(s))
                       for k, s in enumerate(kinds)])
    want_shapes = np.array([(1, 1), (3, 5), (2, 63), (0, 0), (7, 2)], dtype=np.int32)
    want_status = np.array([OK, OK, OK, UNSUPPORTED, OK], dtype=np.uint8)
    at = torch.from_numpy(idx).to(cuda)
    assert torch.equal(status, torch.from_numpy(want_status).to(cuda)[at])
    assert torch.equal(shapes, torch.from_numpy(want_shapes).to(cuda)[at])
    assert torch.equal(raw.view(torch.int32), torch.from_numpy(frames).to(cuda).view(torch.int32)[at])


def _alerts(stamps):
    keys = ("cutoutScience", "cutoutTemplate", "cutoutDifference")
    return [{k: {"stampData": s} for k, s in zip(keys, stamps[i:i + 3])} for i in range(0, len(stamps), 3)]


def _same_triplets(got, want):
    assert torch.equal(got[1].cpu(), want[1].cpu())
    a, b = got[0].cpu().numpy(), want[0].cpu().numpy()
    assert a.shape == b.shape and a.tobytes() == b.tobytes()


def test_whole_path_equals_the_host_path(cuda):
    valid = [s for _, s in valid_corpus()]
    stamps = valid[:21]
    want = alert_utils.make_triplets(_alerts(stamps), device=cuda)
    assert want[0].shape == (7, 3, 63, 63)
    got = alert_utils.make_triplets(_alerts(stamps), device=cuda, decode="device")
    _same_triplets(got, want)
    _same_triplets(alert_utils.make_triplets(_alerts(stamps), device=cuda, decode="device", fallback=None), want)
    # two deferred stamps, in alerts 1 and 5: the host reads both (scaled int16 and float64 images)
    deferred = dict(deferred_corpus())
    mixed = list(stamps)
    mixed[4], mixed[17] = deferred["bitpix16_scaled"], deferred["bitpix-64"]
    want = alert_utils.make_triplets(_alerts(mixed), device=cuda)
    got = alert_utils.make_triplets(_alerts(mixed), device=cuda, decode="device", fallback="host", return_status=True)
    _same_triplets(got, want)
    expect = np.zeros((7, 3), dtype=np.uint8)
    expect[1, 1] = expect[5, 2] = UNSUPPORTED
    assert np.array_equal(got[2].cpu().numpy(), expect)
    trip, drop, st = alert_utils.make_triplets(_alerts(mixed), device=cuda, decode="device", fallback=None,
                                               return_status=True)
    assert np.array_equal(st.cpu().numpy(), expect)
    want_drop = want[1].cpu().numpy().copy()
    assert not want_drop[[1, 5]].any()
    want_drop[[1, 5]] = True
    assert np.array_equal(drop.cpu().numpy(), want_drop)
    keep = np.array([0, 2, 3, 4, 6])
    assert trip.cpu().numpy()[keep].tobytes() == want[0].cpu().numpy()[keep].tobytes()
    # errors surface as on the host path
    mixed[4] = dict((n, s) for n, s, _ in malformed_corpus())["cut_in_body"]
    with pytest.raises(Exception) as host_err:
        alert_utils.make_triplets(_alerts(mixed), device=cuda)
    with pytest.raises(type(host_err.value)):
        alert_utils.make_triplets(_alerts(mixed), device=cuda, decode="device")


def test_empty_batch(cuda):
    raw, shapes, status = alert_utils.decode_stamps_device([], cuda)
    assert raw.shape == (0, 63, 63) and shapes.shape == (0, 2) and status.shape == (0,)
    trip, drop = alert_utils.make_triplets([], device=cuda, decode="device")
    assert trip.shape == (0, 3, 63, 63) and drop.shape == (0,) and drop.dtype == torch.bool
    assert alert_utils.make_triplets([], device=cuda, decode="device", fallback=None, return_status=True)[2].shape == (0, 3)


def test_fallback_none_reads_nothing_back():
    """See the module docstring: the only host read of make_triplets' device path is behind `if fallback == "host"`."""
    reads = (".item(", ".cpu(", ".tolist(", ".numpy(", "nonzero", "synchronize", "bool(")
    src = inspect.getsource(alert_utils.decode_stamps_device)
    assert not any(r in src.split('"""')[2] for r in reads)
    body = inspect.getsource(alert_utils.make_triplets).split('"""')[2]
    device_path = body[body.index("stamps = ["):]
    guarded = device_path[device_path.index('if fallback == "host":'):device_path.index("status = status.view")]
    rest = device_path.replace(guarded, "")
    assert ".cpu(" in guarded and not any(r in rest for r in reads)


def test_malformed_stamps_keep_their_status(cuda):
    """The fixed twelve of the host corpus, mixed with valid stamps: the statuses the host program gives."""
    bad = malformed_corpus()
    good = stamp(_images()[0][:9, :12])
    stamps, want = [], []
    for _, s, st in bad:
        stamps += [s, good]
        want += [st, OK]
    raw, shapes, status = _decode(stamps, cuda)
    assert list(status) == want
    assert not raw[0::2].view(np.uint32).any() and not shapes[0::2].any()
    assert (shapes[1::2] == (9, 12)).all()
    assert same_bits(raw[1], frame_of(alert_utils.decode_stamp(good)))
