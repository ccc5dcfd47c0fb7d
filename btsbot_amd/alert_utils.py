"""Alert packets -> model inputs (the reference's alert_utils.py: make_triplet :110-196, prep_alerts :333-441).

    triplets, drop = make_triplets(alerts, device="cuda")                       # image_input    [N,3,63,63]
    meta = make_metadata(alerts, metadata_cols, new_drb=drb, device="cuda")     # metadata_input [N,len(cols)]
    scores = torch.sigmoid(model(image_input=triplets[~drop], metadata_input=meta[~drop]))

Images.  ``make_triplet`` there gunzips and FITS-decodes the three stamps of an alert on the host (astropy),
then masks NaNs, L2-normalises, flags corrupted stamps and pads to 63x63.  Here the decoding is by default a
dependency-free host step (``decode_stamp``: gzip + the primary HDU of a FITS image -- ZTF cutouts are
single-HDU BITPIX = -32 images) and everything after it is one kernel (``btsbot_prep_triplets``) over a
whole night's batch, writing the float32 NCHW tensor the classifier consumes
(inference_example.py:62-64) without the float64 NHWC detour.  ``make_triplets(..., decode="device")`` runs the
decoding on the GPU as well (``decode_stamps_device``: one upload, one launch of ``btsbot_decode_stamps``).

    # from stamps decoded elsewhere:
    raw, shapes = stack_stamps(list_of_(science, template, difference)_arrays)
    triplets, drop = prep_triplets(raw.cuda(), shapes.cuda())

Metadata.  Six of the 25 columns the shipped multi-modal configurations read (``age``, ``days_since_peak``,
``days_to_peak``, ``peakmag_so_far``, ``maxmag_so_far``, ``nnotdet``) are not packet fields: ``prep_alerts`` there
derives them (and ``peakmag``, ``maxmag``) per object from the light curve so far, in a pandas loop that is quadratic
per object.  Here they are ``CUSTOM_COLS``, one kernel over the whole batch (``btsbot_alert_features``) behind a
stable device sort of the object ids; ``make_metadata`` adds the packet fields and orders the columns.

    feats = alert_features(object_id, jd, magpsf, jdstarthist, ncovhist, ndethist)   # device tensors -> [N,8] float32

Alerts of one object with equal ``jd`` are ordered by input position (the reference's unstable sort leaves that open).

On a live stream a call holds only tonight's alerts of each object: ``make_metadata(..., state=FeatureState(...))``
continues the light curves from a per-object state on the device (features.py), keyed by ``object_keys(objectId)``.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

_FITS_DTYPES = {8: ">u1", 16: ">i2", 32: ">i4", 64: ">i8", -32: ">f4", -64: ">f8"}


def decode_fits_image(buf: bytes) -> np.ndarray:
    """Primary-HDU image of an (uncompressed) FITS file as astropy's ``hdu[0].data`` returns it: shape
    (NAXIS2, NAXIS1) -- NAXIS1 is the fastest axis --, big-endian samples converted to native order,
    BSCALE / BZERO applied when present.  Raises ValueError on anything that is not a 2-D image HDU."""
    cards = {}
    pos, end = 0, None
    while end is None:
        block = buf[pos:pos + 2880]
        if len(block) < 2880:
            raise ValueError("FITS header: END card not found")
        for i in range(0, 2880, 80):
            card = block[i:i + 80].decode("ascii", "replace")
            key = card[:8].strip()
            if key == "END":
                end = pos + 2880
                break
            if card[8:10] == "= ":
                val = card[10:].split("/", 1)[0].strip() if not card[10:].lstrip().startswith("'") \
                    else card[10:].strip().split("'")[1]
                cards[key] = val
        pos += 2880
    try:
        if cards.get("SIMPLE", "T") not in ("T", "t") or int(cards["NAXIS"]) != 2:
            raise ValueError(f"FITS: not a 2-D primary image (NAXIS={cards.get('NAXIS')})")
        bitpix, nx, ny = int(cards["BITPIX"]), int(cards["NAXIS1"]), int(cards["NAXIS2"])
        dt = np.dtype(_FITS_DTYPES[bitpix])
    except KeyError as e:
        raise ValueError(f"FITS header: missing or unsupported {e}") from None
    nbytes = nx * ny * dt.itemsize
    if len(buf) < end + nbytes:
        raise ValueError("FITS: data unit shorter than the header says")
    data = np.frombuffer(buf, dtype=dt, count=nx * ny, offset=end).reshape(ny, nx)
    bscale, bzero = float(cards.get("BSCALE", 1.0)), float(cards.get("BZERO", 0.0))
    if bscale != 1.0 or bzero != 0.0:
        return data.astype(np.float64 if bitpix in (32, 64, -64) else np.float32) * bscale + bzero
    return data.astype(dt.newbyteorder("="))


def decode_stamp(stamp_data) -> np.ndarray:
    """``alert['cutoutScience']['stampData']`` -> the cutout array: gunzip, then the FITS primary image
    (alert_utils.py:139-145 without astropy)."""
    import gzip
    return decode_fits_image(gzip.decompress(bytes(stamp_data)))


def decode_alert(alert) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(science, template, difference) cutouts of one alert packet, in make_triplet's channel order."""
    return tuple(decode_stamp(alert[f"cutout{c}"]["stampData"]) for c in ("Science", "Template", "Difference"))


_STAMP_KEYS = ("cutoutScience", "cutoutTemplate", "cutoutDifference")
STAMP_STATUS = _lib.STAMP_STATUS


def _cuda_device(device, what: str) -> torch.device:
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"btsbot_amd.alert_utils.{what} runs on the GPU; there is no CPU fallback (device is {dev})")
    return dev


def decode_stamps_device(stamps, device="cuda") -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``stampData`` fields (a sequence of bytes-like objects) -> (raw [n,63,63] float32, shapes [n,2] int32 = (h, w),
    status [n] uint8) on ``device``: gunzip and FITS decode of the whole batch in one launch (``btsbot_decode_stamps``).

    raw holds each image in native float32 in the top-left h x w corner, zero elsewhere -- ``stack_stamps``' layout, so
    ``raw.view(-1, 3, 63, 63)`` / ``shapes.view(-1, 3, 2)`` go straight into ``prep_triplets``.  ``status`` is one of
    ``STAMP_STATUS`` per stamp; a stamp with a non-zero status has an all-zero image and shape (0, 0).  The device decodes
    a single gzip member (stored, fixed and dynamic deflate blocks) that inflates to at most 28,800 bytes and holds a
    FITS primary image with SIMPLE = T, NAXIS = 2, BITPIX = -32, axes of 1 .. 63, no BSCALE / BZERO; anything else that is
    well formed is ``UNSUPPORTED`` and left to ``decode_stamp``.  Unlike ``gzip.decompress`` it does not verify the CRC32
    of the gzip trailer (it does verify ISIZE).

    One ``b"".join``, one upload (offsets and bytes in one buffer), one launch; nothing is read back."""
    dev = _cuda_device(device, "decode_stamps_device")
    stamps = list(stamps)
    for i, s in enumerate(stamps):
        if not isinstance(s, (bytes, bytearray, memoryview)):
            raise TypeError(f"stamps[{i}] must be bytes-like, got {type(s).__name__}")
    n = len(stamps)
    if n >= 2 ** 31:
        raise ValueError(f"{n} stamps in one call: more than an int32 counts")
    raw = torch.empty((n, 63, 63), dtype=torch.float32, device=dev)
    shapes = torch.empty((n, 2), dtype=torch.int32, device=dev)
    status = torch.empty(n, dtype=torch.uint8, device=dev)
    if n == 0:
        return raw, shapes, status
    blob = b"".join(stamps)
    head = 8 * (n + 1)
    host = np.empty(head + len(blob), dtype=np.uint8)
    offsets = host[:head].view(np.int64)
    offsets[0] = 0
    np.cumsum([len(s) for s in stamps], out=offsets[1:])
    host[head:] = np.frombuffer(blob, dtype=np.uint8)
    buf = torch.from_numpy(host).to(dev)
    L = _lib.lib()
    ws_bytes = _lib.check(L.btsbot_decode_stamps_workspace(n), "btsbot_decode_stamps_workspace")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(L.btsbot_decode_stamps(
            C.c_void_p(buf.data_ptr() + head), C.c_void_p(buf.data_ptr()), n, C.c_void_p(raw.data_ptr()),
            C.c_void_p(shapes.data_ptr()), C.c_void_p(status.data_ptr()), C.c_void_p(ws.data_ptr()), ws_bytes,
            C.c_void_p(st)), "btsbot_decode_stamps")
    return raw, shapes, status


def make_triplets(alerts, device="cuda", normalize: bool = True, decode: str = "host", fallback: Optional[str] = "host",
                  return_status: bool = False):
    """make_triplet (alert_utils.py:110-196) over a batch of alert packets: the decode, then the arithmetic on
    ``device`` in one launch.  Returns (triplets [B,3,63,63] float32 NCHW, drop [B] bool).

    decode="host" (the default): ``decode_stamp`` per stamp in a Python loop.  decode="device": the three ``stampData``
    fields of every alert go through ``decode_stamps_device`` (its docstring names what the device decodes and that it
    does not verify the gzip CRC32).  Then ``fallback`` says what becomes of a stamp whose status is not 0:
      "host"  one host read of the statuses; those stamps are decoded by ``decode_stamp`` and patched in before
              ``prep_triplets``, so the result is the host path's and errors surface as they do there;
      None    no host synchronisation at all: the alert comes back with ``drop = True``.
    return_status=True adds a third value, the uint8 [B,3] statuses of the device decode (zeros for decode="host")."""
    if decode not in ("host", "device"):
        raise ValueError(f"decode must be 'host' or 'device', got {decode!r}")
    if fallback not in ("host", None):
        raise ValueError(f"fallback must be 'host' or None, got {fallback!r}")
    if decode == "host":
        raw, shapes = stack_stamps([decode_alert(a) for a in alerts])
        out = prep_triplets(raw.to(device), shapes.to(device), normalize)
        if return_status:
            out += (torch.zeros((raw.shape[0], 3), dtype=torch.uint8, device=out[0].device),)
        return out
    stamps = [a[k]["stampData"] for a in alerts for k in _STAMP_KEYS]
    raw, shapes, status = decode_stamps_device(stamps, device)
    if fallback == "host":
        for i in torch.nonzero(status.cpu()).reshape(-1).tolist():
            stamp = decode_stamp(stamps[i])
            h, w = stamp.shape
            if h > 63 or w > 63:
                raise ValueError(f"stamp larger than 63x63: {stamp.shape}")
            frame = np.zeros((63, 63), dtype=np.float32)
            frame[:h, :w] = stamp
            raw[i] = torch.from_numpy(frame).to(raw.device)
            shapes[i] = torch.tensor([h, w], dtype=torch.int32).to(raw.device)
    status = status.view(-1, 3)
    triplets, drop = prep_triplets(raw.view(-1, 3, 63, 63), shapes.view(-1, 3, 2), normalize)
    if fallback is None:
        drop = drop | (status != 0).any(dim=1)
    return (triplets, drop, status) if return_status else (triplets, drop)


def stack_stamps(alerts: Sequence[Sequence[np.ndarray]]) -> Tuple[torch.Tensor, torch.Tensor]:
    """Host helper: decoded stamps (each up to 63x63, any float dtype) -> raw [B,3,63,63] float32 with
    every stamp in the top-left corner + shapes int32 [B,3,2]."""
    n = len(alerts)
    raw = np.zeros((n, 3, 63, 63), dtype=np.float32)
    shapes = np.zeros((n, 3, 2), dtype=np.int32)
    for i, trip in enumerate(alerts):
        if len(trip) != 3:
            raise ValueError("every alert needs (science, template, difference) stamps")
        for c, stamp in enumerate(trip):
            h, w = stamp.shape
            if h > 63 or w > 63:
                raise ValueError(f"stamp larger than 63x63: {stamp.shape}")
            raw[i, c, :h, :w] = stamp
            shapes[i, c] = (h, w)
    return torch.from_numpy(raw), torch.from_numpy(shapes)


def prep_triplets(raw: torch.Tensor, shapes: Optional[torch.Tensor] = None,
                  normalize: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """(triplets [B,3,63,63] float32, drop [B] bool) on raw's device."""
    if raw.device.type != "cuda":
        raise RuntimeError("btsbot_amd.alert_utils.prep_triplets runs on the GPU; there is no CPU "
                           f"fallback (raw is on {raw.device})")
    if raw.dim() != 4 or tuple(raw.shape[1:]) != (3, 63, 63):
        raise ValueError(f"raw must be [B,3,63,63], got {tuple(raw.shape)}")
    raw = raw.to(torch.float32).contiguous()
    b = raw.shape[0]
    if shapes is not None:
        shapes = shapes.to(device=raw.device, dtype=torch.int32).contiguous()
        if tuple(shapes.shape) != (b, 3, 2):
            raise ValueError(f"shapes must be [{b},3,2], got {tuple(shapes.shape)}")
    out = torch.empty_like(raw)
    drop = torch.zeros(b, dtype=torch.uint8, device=raw.device)
    if b == 0:
        return out, drop.bool()
    with torch.cuda.device(raw.device):
        st = torch.cuda.current_stream(raw.device).cuda_stream
        _lib.check(_lib.lib().btsbot_prep_triplets(
            C.c_void_p(raw.data_ptr()), C.c_void_p(shapes.data_ptr() if shapes is not None else 0),
            C.c_void_p(out.data_ptr()), C.c_void_p(drop.data_ptr()), b, int(normalize),
            C.c_void_p(st)), "btsbot_prep_triplets")
    return out, drop.bool()


# ---- metadata: the custom columns of prep_alerts (alert_utils.py:333-441) -----------------------------
# the columns of alert_features(), in its output order
CUSTOM_COLS = ("peakmag", "maxmag", "peakmag_so_far", "maxmag_so_far", "age", "days_since_peak", "days_to_peak",
               "nnotdet")
# alerts per LDS tile of the per-object kernels btsbot_alert_features, btsbot_split_labels and btsbot_policy_eval (TILE in
# csrc/object_walk.h): objects of up to 64 alerts take one wave, up to OBJECT_TILE one workgroup with the object
# resident in LDS, larger ones stream through the tile
OBJECT_TILE = 1024
FEATURE_TILE = OBJECT_TILE
_FEATURE_INPUTS = ("jd", "magpsf", "jdstarthist", "ncovhist", "ndethist")


def _group_by_object(object_id: torch.Tensor,
                     then_by: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(perm int32 [n], seg_offsets int32 [n + 1]) for btsbot_alert_features, on the device and without a host
    sync.  Grouping is plumbing: a stable sort keeps input order inside an object, and object k's run starts where k
    run heads lie to the left.  The number of objects would cost a sync, so the kernel is given n possibly empty
    objects: the offsets past the last object all equal n.  With ``then_by`` (btsbot_trigger_update: jd) an object's
    run is ordered by (then_by, input position): two stable sorts, the minor key first."""
    n, dev = object_id.shape[0], object_id.device
    if then_by is None:
        ids, perm = torch.sort(object_id.to(torch.int64), stable=True)
    else:
        minor = torch.sort(then_by, stable=True).indices
        ids, major = torch.sort(object_id.to(torch.int64)[minor], stable=True)
        perm = minor[major]
    run = torch.zeros(n, dtype=torch.int64, device=dev)
    run[1:] = torch.cumsum(ids[1:] != ids[:-1], 0)
    offsets = torch.searchsorted(run, torch.arange(n + 1, device=dev))
    return perm.to(torch.int32), offsets.to(torch.int32)


def _check_table(where: str, object_id: torch.Tensor, **cols) -> int:
    """The number of alerts n, after the checks every per-object wrapper makes: object_id on the GPU (``where`` names
    the caller, ``module.function``), one-dimensional and of an integer type, every column (None: absent) of shape [n]."""
    if object_id.device.type != "cuda":
        raise RuntimeError(f"btsbot_amd.{where} runs on the GPU; there is no CPU fallback (object_id is on "
                           f"{object_id.device})")
    if object_id.dim() != 1:
        raise ValueError(f"object_id must be one-dimensional, got {tuple(object_id.shape)}")
    n = object_id.shape[0]
    for name, t in cols.items():
        if t is not None and (t.dim() != 1 or t.shape[0] != n):
            raise ValueError(f"{name} must be [{n}], got {tuple(t.shape)}")
    if object_id.dtype.is_floating_point or object_id.dtype == torch.bool:
        raise ValueError(f"object_id must be an integer tensor, got {object_id.dtype}")
    return n


def _launch_grouped(symbol: str, grouping: Tuple[torch.Tensor, torch.Tensor], n: int, *args) -> None:
    """One launch of a per-object kernel (csrc/object_walk.h) on the current stream of the grouping's device:
    ``symbol(perm, seg_offsets, n, n, *args, stream)`` with ``grouping`` = ``_group_by_object``'s result -- n alerts in n
    possibly empty objects.  Tensors among ``args`` go as their device pointers.  No host synchronisation."""
    def ptr(a):
        return C.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else a

    dev = grouping[0].device
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(getattr(_lib.lib(), symbol)(*map(ptr, grouping), n, n, *map(ptr, args), C.c_void_p(st)), symbol)


def alert_features(object_id: torch.Tensor, jd: torch.Tensor, magpsf: torch.Tensor, jdstarthist: torch.Tensor,
                   ncovhist: torch.Tensor, ndethist: torch.Tensor) -> torch.Tensor:
    """CUSTOM_COLS of N alerts as float32 [N, 8] on the inputs' device, rows in input order.

    object_id: any integers (equal = same object); jd, magpsf, jdstarthist are taken as float64, ncovhist, ndethist as
    int32.  With O(i) the alerts of i's object and P(i) those of them up to and including i in (jd, input position)
    order: peakmag / maxmag = min / max magpsf over O(i), *_so_far over P(i); age = jd - first, days_since_peak = jd -
    jdpk, days_to_peak = jdpk - first with first = min(jdstarthist[i], min jd over O(i)) and jdpk the jd of the
    earliest alert of P(i) at peakmag_so_far; nnotdet = ncovhist - ndethist.  NaN magpsf are skipped (all NaN: NaN); a
    NaN jdstarthist gives NaN age and days_to_peak.  jd must be finite (not checked: that would be a host sync).
    Everything is compared and subtracted in float64 and rounded to float32 once.  No host synchronisation."""
    n = _check_table("alert_utils.alert_features", object_id, jd=jd, magpsf=magpsf, jdstarthist=jdstarthist,
                     ncovhist=ncovhist, ndethist=ndethist)
    dev = object_id.device
    jd, magpsf, jdstarthist = (t.to(device=dev, dtype=torch.float64).contiguous() for t in (jd, magpsf, jdstarthist))
    ncovhist, ndethist = (t.to(device=dev, dtype=torch.int32).contiguous() for t in (ncovhist, ndethist))
    out = torch.empty((n, 8), dtype=torch.float32, device=dev)
    if n:
        _launch_grouped("btsbot_alert_features", _group_by_object(object_id), n,
                        jd, magpsf, jdstarthist, ncovhist, ndethist, out)
    return out


_ZTF_LETTERS = 7
_ZTF_YEAR = 26 ** _ZTF_LETTERS


def object_keys(names) -> np.ndarray:
    """A stable int64 id per ``objectId`` string, so that one object keeps its slot in a ``FeatureState`` or
    ``TriggerState`` across calls (and across processes).  ``ZTF`` + two digits + seven letters a-z encodes exactly and
    reversibly as yy * 26**7 + the letters read as a base-26 number (``object_names`` inverts it); any other string
    becomes -(1 + h % (2**63 - 1)) with h the 8-byte blake2b digest of its UTF-8 bytes read as an unsigned big-endian
    integer: negative, so it cannot collide with a ZTF code, and never the states' reserved id -2**63."""
    import hashlib
    out = np.empty(len(names), dtype=np.int64)
    for i, name in enumerate(names):
        name = str(name)
        tail = name[5:]
        if (len(name) == 5 + _ZTF_LETTERS and name.startswith("ZTF") and name[3:5].isascii() and name[3:5].isdigit()
                and all("a" <= c <= "z" for c in tail)):
            code = 0
            for c in tail:
                code = code * 26 + (ord(c) - ord("a"))
            out[i] = int(name[3:5]) * _ZTF_YEAR + code
        else:
            h = int.from_bytes(hashlib.blake2b(name.encode("utf-8"), digest_size=8).digest(), "big")
            out[i] = -(1 + h % (2 ** 63 - 1))
    return out


def object_names(keys) -> list:
    """The ZTF names of ``object_keys``' exact codes; a key outside 0 .. 100 * 26**7 - 1 (a hashed name) raises
    ValueError."""
    names = []
    for key in np.asarray(keys, dtype=np.int64).reshape(-1).tolist():
        if not 0 <= key < 100 * _ZTF_YEAR:
            raise ValueError(f"{key} is not the code of a ZTF name")
        yy, code = divmod(key, _ZTF_YEAR)
        letters = []
        for _ in range(_ZTF_LETTERS):
            code, r = divmod(code, 26)
            letters.append(chr(ord("a") + r))
        names.append(f"ZTF{yy:02d}" + "".join(reversed(letters)))
    return names


def make_metadata(alerts, metadata_cols: Sequence[str], new_drb=None, device="cuda", state=None) -> torch.Tensor:
    """metadata_input [N, len(metadata_cols)] float32 on ``device`` for alert packets as prep_alerts
    (alert_utils.py:333-441) takes them, columns in the order of ``metadata_cols``.

    Each alert's row is ``alert["candidate"] | alert.get("classifications", {})``.  A column is, in this order of
    precedence (the order in which prep_alerts overwrites the frame): one of CUSTOM_COLS, computed on the device from
    objectId / jd / magpsf / jdstarthist / ncovhist / ndethist; ``"new_drb"`` when ``new_drb`` (one score per alert,
    the caller's, as it is an argument of prep_alerts) is given; a packet field (of any alert: absent elsewhere = NaN,
    as in a DataFrame; None = NaN).  Anything else raises KeyError naming the column, before any device work.

    state: a ``FeatureState`` on ``device``.  Without one the custom columns come from ``alert_features`` over the alerts
    of this call.  With one they come from ``state.update`` on ``object_keys`` of the packets' objectIds, so they continue
    each object's light curve from the calls before: the six causal columns are what one call over the whole stream
    would give, ``peakmag`` / ``maxmag`` are the so-far values, and the rows of alerts the state dropped (table full)
    carry NaN in every custom column."""
    alerts = list(alerts)
    cols = list(metadata_cols)
    n = len(alerts)
    rows = [a["candidate"] | a.get("classifications", {}) for a in alerts]
    fields = set().union(*rows) if rows else set()
    custom = [c for c in cols if c in CUSTOM_COLS]
    if new_drb is not None:
        new_drb = np.asarray(new_drb, dtype=np.float64).reshape(-1)
        if new_drb.shape[0] != n:
            raise ValueError(f"new_drb has {new_drb.shape[0]} scores for {n} alerts")
    for c in cols:
        if n and c not in CUSTOM_COLS and not (c == "new_drb" and new_drb is not None) and c not in fields:
            raise KeyError(c)
    for c in (_FEATURE_INPUTS if custom and n else ()):
        if c not in fields:
            raise KeyError(c)

    def column(name, dtype=np.float64):
        vals = [r.get(name) for r in rows]
        return np.array([np.nan if v is None else v for v in vals], dtype=dtype)

    host = np.zeros((n, len(cols)), dtype=np.float32)
    for k, c in enumerate(cols):
        if c in CUSTOM_COLS:
            continue
        host[:, k] = new_drb if (c == "new_drb" and new_drb is not None) else column(c)
    if custom and n:
        if state is None:
            ids = {}
            object_id = np.array([ids.setdefault(a["objectId"], len(ids)) for a in alerts], dtype=np.int64)
        else:
            object_id = object_keys([a["objectId"] for a in alerts])
        jd = column("jd")
        if not np.isfinite(jd).all():
            raise ValueError("make_metadata: every alert needs a finite candidate.jd")
        try:
            ncov, ndet = column("ncovhist", np.int32), column("ndethist", np.int32)
        except ValueError:
            raise ValueError("make_metadata: every alert needs integer ncovhist and ndethist") from None
        feats_in = [torch.from_numpy(x).to(device) for x in
                    (object_id, jd, column("magpsf"), column("jdstarthist"), ncov, ndet)]
    out = torch.from_numpy(host).to(device)
    if custom and n:
        feats = alert_features(*feats_in) if state is None else state.update(*feats_in)["features"]
        dst = torch.tensor([k for k, c in enumerate(cols) if c in CUSTOM_COLS], device=out.device)
        src = torch.tensor([CUSTOM_COLS.index(c) for c in cols if c in CUSTOM_COLS], device=out.device)
        out[:, dst] = feats[:, src]
    return out
