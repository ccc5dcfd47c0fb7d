"""The rules of btsbot_decode_stamps on the host: csrc/inflate_core.h compiled into tools/unit/stamp_decode_check.cpp and
run over a corpus of valid stamps, the deferred cases and 2,000 seeded mutants.  No GPU.

The stamps come from the writer in this module (gzip of a single-HDU FITS file: 80-character cards, big-endian data,
2880-byte padding; the gzip member is assembled by hand around zlib's raw deflate so that every header flag, strategy and
window size can be chosen).  The oracle is never the code under test: Python's zlib for the container, and
alert_utils.decode_stamp / decode_fits_image for the image.  tests/test_gpu_stamp_decode.py submits the same corpus to
the kernel.

Mutants.  The issue's rule -- status 0 if and only if zlib inflates the deflate body completely, within the cap, with
matching ISIZE and nothing after the trailer -- is a statement about the container (gzip header, deflate stream,
trailer), so it is asserted on the program's CONTAINER status, with the inflated bytes equal to zlib's.  A byte flip
inside a stored block leaves the container valid and may break the FITS header it carries; the final status is
therefore held to its own oracle: 0 only if decode_fits_image reads zlib's bytes as a float32 image of the same
shape and bit pattern."""
import os
import re
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

from btsbot_amd import _lib, alert_utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 28800
OK, BAD_GZIP, BAD_DEFLATE, TOO_LARGE, BAD_TRAILER, BAD_FITS, UNSUPPORTED = range(7)


# ---- the writer -------------------------------------------------------------------------------------------------------------
def _card(key, value, comment=None):
    text = f"{key:<8}= {value:>20}"
    if comment is not None:
        text += f" / {comment}"
    assert len(text) <= 80
    return text.ljust(80)


def fits_bytes(img, bitpix=-32, extra=(), simple="T", comment=False, filler=0, end=True, data_bytes=None):
    """A single-HDU FITS file of the 2-D array `img` (rows = NAXIS2).  extra: more (key, value) cards; filler: that many
    HISTORY cards (37+ cards make a two-block header); end=False leaves the END card out; data_bytes cuts the data."""
    dt = {-32: ">f4", -64: ">f8", 16: ">i2", 32: ">i4"}[bitpix]
    h, w = img.shape
    cards = [_card("SIMPLE", simple, "conforms to FITS" if comment else None), _card("BITPIX", bitpix),
             _card("NAXIS", 2, "two axes" if comment else None), _card("NAXIS1", w), _card("NAXIS2", h)]
    cards += [_card(k, v) for k, v in extra]
    cards += [f"HISTORY filler card {i}".ljust(80) for i in range(filler)]
    if end:
        cards.append("END".ljust(80))
    header = "".join(cards).encode("ascii")
    header += b" " * (-len(header) % 2880)
    data = np.ascontiguousarray(img, dtype=dt).tobytes()
    data += b"\0" * (-len(data) % 2880)
    return header + (data if data_bytes is None else data[:data_bytes])


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15, flush_at=None):
    c = zlib.compressobj(level, zlib.DEFLATED, -wbits, 8, strategy)
    if flush_at is None:
        return c.compress(data) + c.flush()
    return c.compress(data[:flush_at]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(data[flush_at:]) + c.flush()


def gz_member(data, body=None, fname=None, fextra=None, fcomment=None, fhcrc=False, **kw):
    """One gzip member (RFC 1952) of `data`; `body` replaces the deflate stream (hand-made streams)."""
    flg = (2 if fhcrc else 0) | (4 if fextra is not None else 0) | (8 if fname is not None else 0) | \
        (16 if fcomment is not None else 0)
    head = b"\x1f\x8b\x08" + bytes([flg]) + struct.pack("<IBB", 1_600_000_000, 2, 3)
    if fextra is not None:
        head += struct.pack("<H", len(fextra)) + fextra
    if fname is not None:
        head += fname + b"\0"
    if fcomment is not None:
        head += fcomment + b"\0"
    if fhcrc:
        head += struct.pack("<H", zlib.crc32(head) & 0xffff)
    body = deflate(data, **kw) if body is None else body
    return head + body + struct.pack("<II", zlib.crc32(data) & 0xffffffff, len(data) & 0xffffffff)


def stamp(img, gz=None, **fits):
    return gz_member(fits_bytes(np.asarray(img), **fits), **(gz or {}))


def _images():
    rng = np.random.default_rng(11)
    noise = rng.standard_normal((63, 63)).astype(np.float32) * 30 + 100
    ramp = (np.arange(63, dtype=np.float32)[:, None] * 0.5 + np.arange(63, dtype=np.float32)[None, :] * 0.25)
    special = noise.copy()
    special[0, 0], special[5, 7], special[62, 62], special[30, :3] = np.nan, np.inf, -np.inf, np.nan
    return noise, np.full((63, 63), 7.25, dtype=np.float32), ramp, special


def valid_corpus():
    """[(name, stamp bytes)]: every one must decode on the device path."""
    noise, const, ramp, special = _images()
    out = []
    for level in (0, 1, 6, 9):
        out.append((f"level{level}", stamp(noise, dict(level=level))))
    for name, strat in (("fixed", zlib.Z_FIXED), ("huffman_only", zlib.Z_HUFFMAN_ONLY), ("rle", zlib.Z_RLE)):
        for iname, img in (("noise", noise), ("const", const), ("ramp", ramp)):
            out.append((f"{name}_{iname}", stamp(img, dict(strategy=strat))))
    out.append(("full_flush", stamp(noise, dict(flush_at=9000))))
    out.append(("full_flush_ramp", stamp(ramp, dict(flush_at=2880))))
    for wbits in (9, 15):
        out.append((f"wbits{wbits}", stamp(ramp, dict(wbits=wbits, level=9))))
    out.append(("fname", stamp(noise, dict(fname=b"cutout.fits"))))
    out.append(("fextra", stamp(noise, dict(fextra=b"AP\x04\x00abcd"))))
    out.append(("fcomment", stamp(noise, dict(fcomment=b"science cutout"))))
    out.append(("fhcrc", stamp(noise, dict(fhcrc=True))))
    out.append(("all_flags", stamp(ramp, dict(fname=b"a.fits", fextra=b"\x01\x02", fcomment=b"c", fhcrc=True))))
    for iname, img in (("noise", noise), ("const", const), ("ramp", ramp), ("nan_inf", special)):
        out.append((f"content_{iname}", stamp(img)))
    for h, w in ((63, 63), (63, 40), (40, 63), (62, 63), (1, 1)):
        out.append((f"shape_{h}x{w}", stamp(special[:h, :w])))
    out.append(("two_block_header", stamp(noise, filler=40)))
    out.append(("card_comment", stamp(ramp[:20, :31], comment=True)))
    return out


def deferred_corpus():
    """[(name, stamp bytes)]: well formed, outside what the device decodes -> UNSUPPORTED."""
    noise, _, ramp, _ = _images()
    i16 = np.arange(35, dtype=np.int16).reshape(5, 7)
    two = stamp(noise[:9, :12]) + stamp(ramp[:9, :12])
    return [("bitpix16_scaled", stamp(i16, bitpix=16, extra=(("BZERO", 32768), ("BSCALE", 2)))),
            ("bitpix-64", stamp(noise[:40, :40].astype(np.float64), bitpix=-64)),
            ("64x63", stamp(np.zeros((64, 63), np.float32) + ramp[:1, :63])),
            ("simple_F", stamp(noise, simple="F")),
            ("two_members", two)]


# ---- hand-made deflate streams -------------------------------------------------------------------------------------------------
class _BitWriter:
    def __init__(self):
        self.bits = []

    def put(self, value, n):           # a field: least significant bit first
        self.bits += [(value >> i) & 1 for i in range(n)]
        return self

    def huff(self, code, n):           # a Huffman code: most significant bit first
        self.bits += [(code >> (n - 1 - i)) & 1 for i in range(n)]
        return self

    def bytes(self):
        bits = self.bits + [0] * (-len(self.bits) % 8)
        return bytes(sum(b << i for i, b in enumerate(bits[k:k + 8])) for k in range(0, len(bits), 8))


def malformed_corpus():
    """The fixed list of twelve: (name, stamp bytes, the status the rules give).  The host test asserts that the host
    program gives these statuses; the GPU test expects the same of the kernel."""
    noise, const, ramp, _ = _images()
    small = noise[:9, :12]
    good = stamp(small)
    body_at = 10
    fits = fits_bytes(small)
    stored = stamp(small, dict(level=0))
    nlen_at = 10 + 3   # stored block: 1 byte of block header, LEN (2), then NLEN
    return [
        ("cut_in_header", good[:5], BAD_GZIP),
        ("cut_in_body", good[:body_at + (len(good) - 18) // 2], BAD_DEFLATE),
        ("cut_in_trailer", good[:-3], BAD_TRAILER),
        ("bad_magic", b"\x1f\x8c" + good[2:], BAD_GZIP),
        ("bad_block_type", gz_member(b"", body=_BitWriter().put(1, 1).put(3, 2).bytes()), BAD_DEFLATE),
        # dynamic block, HLIT = HDIST = 0, 19 code-length codes all of length 1
        ("oversubscribed", gz_member(b"", body=_BitWriter().put(1, 1).put(2, 2).put(0, 5).put(0, 5).put(15, 4)
                                     .put(int("001" * 19, 2), 57).put(0, 16).bytes()), BAD_DEFLATE),
        # fixed block whose first symbol is a match: length 3 (symbol 257 = 0000001), distance 1 (00000)
        ("distance_too_far", gz_member(b"abc", body=_BitWriter().put(1, 1).put(1, 2).huff(1, 7).huff(0, 5).huff(0, 7)
                                       .bytes()), BAD_DEFLATE),
        ("stored_nlen", stored[:nlen_at] + bytes([stored[nlen_at] ^ 0x10]) + stored[nlen_at + 1:], BAD_DEFLATE),
        ("isize_mismatch", good[:-4] + struct.pack("<I", len(fits) + 1), BAD_TRAILER),
        ("over_cap", stamp(np.zeros((63, 63)) + ramp, bitpix=-64), TOO_LARGE),
        ("no_end_card", stamp(small, end=False), BAD_FITS),
        ("short_data_unit", stamp(small, data_bytes=9 * 12 * 4 - 1), BAD_FITS),
    ]


# ---- the oracle ----------------------------------------------------------------------------------------------------------------
def gzip_body_start(m):
    """Where the deflate stream starts (RFC 1952 restated), or None."""
    if len(m) < 10 or m[0] != 0x1f or m[1] != 0x8b or m[2] != 8 or m[3] & 0xe0:
        return None
    flg, pos = m[3], 10
    if flg & 4:
        if len(m) < pos + 2:
            return None
        pos += 2 + m[pos] + 256 * m[pos + 1]
        if pos > len(m):
            return None
    for bit in (8, 16):
        if flg & bit:
            z = m.find(b"\0", pos)
            if z < 0:
                return None
            pos = z + 1
    if flg & 2:
        pos += 2
        if pos > len(m):
            return None
    return pos


def container_oracle(m):
    """The bytes zlib inflates from the member, or None unless: the stream is complete, within the cap, ISIZE matches and
    nothing follows the trailer."""
    start = gzip_body_start(m)
    if start is None:
        return None
    d = zlib.decompressobj(wbits=-15)
    try:
        out = d.decompress(m[start:], CAP + 1)
    except zlib.error:
        return None
    if not d.eof or len(out) > CAP or len(d.unused_data) != 8:
        return None
    return out if struct.unpack("<I", d.unused_data[4:])[0] == len(out) else None


def frame_of(img):
    frame = np.zeros((63, 63), dtype=np.float32)
    frame[:img.shape[0], :img.shape[1]] = img
    return frame


# ---- the program ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or \
        next((p for p in (os.path.join(rocm, "llvm", "bin", "clang++"), os.path.join(rocm, "bin", "amdclang++"))
              if os.path.isfile(p)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("stamp_decode") / "stamp_decode_check")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-Wall", "-o", exe,
                           os.path.join(ROOT, "tools", "unit", "stamp_decode_check.cpp")])
    return exe


def run_program(exe, stamps, workdir):
    """[(container status, status, h, w, inflated bytes or None, frame [63,63] float32 or None)] per stamp."""
    src, dst = os.path.join(str(workdir), "stamps.bin"), os.path.join(str(workdir), "results.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<I", len(stamps)))
        for s in stamps:
            f.write(struct.pack("<I", len(s)) + bytes(s))
    subprocess.run([exe, src, dst], check=True, timeout=120)
    res = open(dst, "rb").read()
    out, pos = [], 0
    for _ in stamps:
        gz, st, h, w, n = struct.unpack_from("<BBiiI", res, pos)
        pos += 14
        data = frame = None
        if gz == OK:
            data = res[pos:pos + n]
            pos += n
        if st == OK:
            frame = np.frombuffer(res, dtype=np.float32, count=63 * 63, offset=pos).reshape(63, 63)
            pos += 63 * 63 * 4
        out.append((gz, st, h, w, data, frame))
    assert pos == len(res)
    return out


def same_bits(got, want):
    """float32 arrays equal as bit patterns where `want` is not NaN, NaN where it is"""
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


# ---- tests ---------------------------------------------------------------------------------------------------------------------
def test_valid_corpus_decodes_as_decode_stamp(program, tmp_path):
    corpus = valid_corpus()
    names = [n for n, _ in corpus]
    assert len(set(names)) == len(names) and len(corpus) == 33
    for (name, s), (gz, st, h, w, data, frame) in zip(corpus, run_program(program, [s for _, s in corpus], tmp_path)):
        want = alert_utils.decode_stamp(s)
        assert want.dtype == np.float32, name
        assert (gz, st) == (OK, OK), (name, gz, st)
        assert data == zlib.decompress(s, wbits=31), name
        assert (h, w) == want.shape, (name, h, w)
        assert same_bits(frame, frame_of(want)), name
    # the corpus is what it says: stored blocks at level 0, a distance set of one code under Z_RLE, two header blocks
    by_name = dict(corpus)
    assert by_name["level0"][10] & 6 == 0 and len(by_name["level0"]) > 20160
    assert len(by_name["content_const"]) < 400
    assert zlib.decompress(by_name["two_block_header"], wbits=31)[2880:2880 + 7] == b"HISTORY"


def test_deferred_cases_are_unsupported(program, tmp_path):
    corpus = deferred_corpus()
    assert [n for n, _ in corpus] == ["bitpix16_scaled", "bitpix-64", "64x63", "simple_F", "two_members"]
    for (name, s), (gz, st, h, w, _, frame) in zip(corpus, run_program(program, [s for _, s in corpus], tmp_path)):
        assert st == UNSUPPORTED and (h, w) == (0, 0) and frame is None, (name, gz, st)
        assert gz == (UNSUPPORTED if name == "two_members" else OK), name
    # the host path reads four of them; SIMPLE = F is refused there as well
    for name, s in corpus:
        if name == "simple_F":
            with pytest.raises(ValueError):
                alert_utils.decode_stamp(s)
        elif name != "64x63":
            assert alert_utils.decode_stamp(s).ndim == 2, name
    assert alert_utils.decode_stamp(dict(corpus)["64x63"]).shape == (64, 63)


def test_the_twelve_malformed_stamps(program, tmp_path):
    corpus = malformed_corpus()
    assert len(corpus) == 12
    got = run_program(program, [s for _, s, _ in corpus], tmp_path)
    assert [(n, r[1]) for (n, _, _), r in zip(corpus, got)] == [(n, st) for n, _, st in corpus]
    for (name, s, _), r in zip(corpus, got):
        assert r[2:4] == (0, 0) and r[5] is None, name
        assert (r[0] == OK) == (container_oracle(s) is not None), name


def _mutants(count=2000, seed=2026):
    """Seeded mutants of valid streams of every block type: cuts at and around every boundary (header end, the
    code-length area, the body, the trailer), and single-byte changes in each of those regions."""
    noise, const, ramp, special = _images()
    rng = np.random.default_rng(seed)
    small = [noise[:9, :12], const[:20, :20], ramp[:13, :7], special[:6, :6]]
    bases = []
    for k, img in enumerate(small):
        for gz in (dict(level=0), dict(level=1), dict(level=6), dict(level=9), dict(strategy=zlib.Z_FIXED),
                   dict(strategy=zlib.Z_HUFFMAN_ONLY), dict(strategy=zlib.Z_RLE), dict(flush_at=3000),
                   dict(fname=b"n.fits", fextra=b"xy", fcomment=b"c", fhcrc=True), dict(wbits=9)):
            bases.append(stamp(img, gz, filler=40 if k == 1 else 0))
    bases.append(stamp(noise, dict(level=6)))       # one full-size stamp: long dynamic blocks
    out = []
    for i in range(count):
        base = bases[i % len(bases)]
        start, n = gzip_body_start(base), len(base)
        regions = {"header": (0, start), "lengths": (start, min(start + 48, n - 8)), "body": (start, n - 8),
                   "trailer": (n - 8, n)}
        kind = ("cut", "flip", "set")[int(rng.integers(0, 3))] if i % 4 else "cut"
        lo, hi = list(regions.values())[int(rng.integers(0, 4))]
        at = int(rng.integers(lo, hi))
        if kind == "cut":
            at = int(rng.choice([at, lo, hi, hi - 1, lo + 1, n - 1, n - 4, n - 8, n - 9]))
            out.append(base[:max(at, 0)])
        elif kind == "flip":
            out.append(base[:at] + bytes([base[at] ^ (1 << int(rng.integers(0, 8)))]) + base[at + 1:])
        else:
            out.append(base[:at] + bytes([int(rng.integers(0, 256))]) + base[at + 1:])
    return out


def test_mutants_against_zlib(program, tmp_path):
    mutants = _mutants()
    assert len(mutants) == 2000
    results = run_program(program, mutants, tmp_path)          # (a crash or a hang fails here)
    accepted = images = 0
    for k, (m, (gz, st, h, w, data, frame)) in enumerate(zip(mutants, results)):
        want = container_oracle(m)
        assert (gz == OK) == (want is not None), (k, gz, len(m))
        if gz != OK:
            assert st == gz and frame is None, k
            continue
        accepted += 1
        assert data == want, k
        try:
            img = alert_utils.decode_fits_image(want)
        except ValueError:
            img = None
        if st == OK:
            assert img is not None and img.dtype == np.float32 and img.shape == (h, w), k
            assert same_bits(frame, frame_of(img)), k
            images += 1
        else:
            assert st in (BAD_FITS, UNSUPPORTED) and (h, w) == (0, 0), (k, st)
    # the corpus exercises both answers
    assert 100 < accepted < 1500 and images > 50, (accepted, images)


def test_python_side_argument_checks():
    with pytest.raises(ValueError, match="decode"):
        alert_utils.make_triplets([], decode="gpu")
    with pytest.raises(ValueError, match="fallback"):
        alert_utils.make_triplets([], decode="device", fallback="device")
    with pytest.raises(TypeError, match=r"stamps\[1\]"):
        alert_utils.decode_stamps_device([b"", "a string"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        alert_utils.decode_stamps_device([b""], device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        alert_utils.make_triplets([], device="cpu", decode="device")
    import inspect
    sig = inspect.signature(alert_utils.make_triplets)
    assert [sig.parameters[k].default for k in ("decode", "fallback", "return_status")] == ["host", "host", False]
    hdr = open(os.path.join(ROOT, "include", "btsbot_hip.h")).read()
    declared = {n: int(v) for n, v in re.findall(r"BTSBOT_STAMP_([A-Z_]+) = (\d+)", hdr)}
    assert declared == _lib.STAMP_STATUS == alert_utils.STAMP_STATUS and len(declared) == 7
    assert int(re.search(r"#define BTSBOT_STAMP_CAP (\d+)", hdr).group(1)) == _lib.STAMP_CAP == CAP


def test_c_abi_argument_checks():
    """Everything btsbot_decode_stamps refuses, it refuses before any HIP call: this runs without a device."""
    import ctypes as C
    L = _lib.lib()
    assert "btsbot_decode_stamps" in _lib.SYMBOLS and "btsbot_decode_stamps_workspace" in _lib.SYMBOLS
    ws = L.btsbot_decode_stamps_workspace
    assert [ws(n) for n in (0, 1, 64, 65, 32768, 10 ** 6)] == [c * CAP for c in (0, 64, 64, 128, 32768, 32768)]
    assert ws(-1) == _lib.ERR_INVALID_ARG
    p = C.c_void_p(64)          # never dereferenced: every call below is refused first
    args = [p, p, 3, p, p, p, p, 64 * CAP, None]
    for k, bad in ((0, None), (1, None), (3, None), (4, None), (5, None), (6, None), (2, -1), (7, 64 * CAP - 1),
                   (6, C.c_void_p(66))):
        a = list(args)
        a[k] = bad
        assert L.btsbot_decode_stamps(*a) == _lib.ERR_INVALID_ARG, k
        assert b"btsbot_decode_stamps" in L.btsbot_last_error(), k
    assert L.btsbot_abi_version() == 1
