"""The host side of mopa_amd/jpegdec.py without a GPU: the numpy restatement tests/_jpeg_reference.py against Pillow (where it can be
imported) and against the fixture tests/golden/g16_jpegdec.npz (always), the library's entropy stage (csrc/jpeg_entropy.h behind
mopa_jpeg_info / mopa_jpeg_coeff_bytes / mopa_jpeg_entropy_decode) against the restatement, every proper prefix of three streams,
the Python layer's argument checks, and the stand-alone sanitizer program tests/jpeg_entropy_check.cpp.  Every comparison is an
equality."""
import ctypes
import io
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest
import torch

import _jpeg_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREFIX_CASES = ("s444_9x16", "s422_17x8", "s420_q10")


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "g16_jpegdec.npz"))


@pytest.fixture(scope="module")
def names(fx):
    return [str(n) for n in fx["names"]]


@pytest.fixture(scope="module")
def jd():
    import __graft_entry__
    from mopa_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        __graft_entry__.build()
    from mopa_amd import jpegdec
    return jpegdec


def stream(fx, name):
    return fx[f"{name}_jpg"].tobytes()


# ------------------------------------------------------------------------------------------------ the restatement
def test_fixture_holds_the_cases_the_issue_names(fx, names):
    assert names == [c[0] for c in ref.small_cases()] and len(names) > 32
    for s, (hs, vs) in (("444", (1, 1)), ("422", (2, 1)), ("420", (2, 2))):
        geoms = [fx[f"{n}_geom"] for n in names if n.startswith(f"s{s}_")]
        assert all((g[3], g[4]) == (hs, vs) and g[2] == 3 for g in geoms)
        assert {int(g[0]) for g in geoms} >= {1, 7, 8, 9, 15, 16, 17, 33, 40} and {int(g[1]) for g in geoms} >= {1, 8, 9, 16, 17, 56}
        assert (fx[f"s{s}_q100_quant"] == 1).all()
        assert fx[f"s{s}_rst1_geom"][5] == 1 and fx[f"s{s}_rst3_geom"][5] == 3
        assert b"\xff\xd0" in stream(fx, f"s{s}_rst1") and b"\xff\xdd" not in stream(fx, f"s{s}_opt")
        assert len(stream(fx, f"s{s}_opt")) < len(stream(fx, f"s{s}_q10")) + 400          # optimised tables are shorter than the default ones
    assert fx["grey_33x17_geom"][2] == 1
    assert fx["full_jpg"].size < 200_000


def test_restatement_reproduces_the_fixture(fx, names):
    for n in names:
        hdr, planes = ref.decode_coefficients(stream(fx, n))
        assert [hdr.width, hdr.height, hdr.ncomp, hdr.hs, hdr.vs, hdr.restart_interval] == fx[f"{n}_geom"].tolist(), n
        assert np.array_equal(hdr.quant, fx[f"{n}_quant"]), n
        for c, p in enumerate(planes):
            assert p.dtype == np.int16 and np.array_equal(p, fx[f"{n}_c{c}"]), (n, c)
        got = ref.pixels(hdr, ref.component_planes(hdr, planes))
        assert got.dtype == np.uint8 and np.array_equal(got, fx[f"{n}_rgb"]), n


def test_restatement_reproduces_pillow_on_fresh_streams():
    Image = pytest.importorskip("PIL.Image")
    k = 0
    for W, H in ((23, 19), (64, 48), (3, 5), (2, 2), (50, 1)):
        for s, sub in ref.SAMPLINGS.items():
            for opts in (dict(quality=85), dict(quality=30, optimize=True), dict(quality=97, restart_marker_blocks=2)):
                buf = io.BytesIO()
                Image.fromarray(ref.synthetic(W, H, 500 + k)).save(buf, "JPEG", subsampling=sub, **opts)
                want = np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))
                assert np.array_equal(ref.decode(buf.getvalue()), want), (W, H, s, opts)
                k += 1
    buf = io.BytesIO()
    Image.fromarray(ref.synthetic(21, 13, 77, gray=True)).save(buf, "JPEG", quality=80)
    assert np.array_equal(ref.decode(buf.getvalue()), np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB")))


def test_restatement_full_size_has_the_recorded_checksums(fx, golden_dir):
    import json
    full = json.load(open(os.path.join(golden_dir, "g16_jpegdec_fullsize.json")))
    got = ref.decode(fx["full_jpg"].tobytes())
    assert list(got.shape) == [full["size"][1], full["size"][0], 3]
    assert zlib.crc32(got.tobytes()) == full["crc32"] and int(got.sum(dtype=np.uint64)) == full["sum"]


def test_restatement_refuses_and_rejects(fx):
    for n in ("refused_progressive", "refused_1x2"):
        with pytest.raises(ref.Unsupported):
            ref.decode(stream(fx, n))
    good = stream(fx, "s420_q10")
    with pytest.raises(ref.DataError):
        ref.decode(good[:-2])
    with pytest.raises(ref.DataError):
        ref.decode(b"\x00" + good)


# ------------------------------------------------------------------------------------------------ the library's entropy stage
def test_entropy_stage_equals_the_restatement(jd, fx, names):
    for n in names + ["full"]:
        data = stream(fx, n)
        want_h, want_p = ref.decode_coefficients(data)
        h, buf = jd.decode_entropy(data)
        assert (h.width, h.height, h.ncomp, h.hs, h.vs, h.restart_interval) == tuple(want_h[:5]) + (want_h.restart_interval,), n
        assert list(h.blocks_x)[:h.ncomp] == list(want_h.blocks_x) and list(h.blocks_y)[:h.ncomp] == list(want_h.blocks_y), n
        assert list(h.comp_w)[:h.ncomp] == list(want_h.comp_w) and list(h.comp_h)[:h.ncomp] == list(want_h.comp_h), n
        assert h.supported == 1 and h.reason == 0 and np.array_equal(h.quant_tables(), want_h.quant), n
        assert buf.dtype == torch.uint8 and buf.numel() == h.coeff_bytes == 384 + sum(p.size for p in want_p) * 2, n
        assert h.plane_off[0] == 384 and all(h.plane_off[c + 1] == h.plane_off[c] + want_p[c].size * 2 for c in range(h.ncomp - 1)), n
        q = buf.numpy()[:384].view(np.uint16).reshape(3, 64)
        assert np.array_equal(q[:h.ncomp], want_h.quant) and not q[h.ncomp:].any(), n
        for c, p in enumerate(jd.coefficient_planes(h, buf)):
            assert np.array_equal(p, want_p[c]), (n, c)
        # the packer is the inverse
        h2, buf2 = jd.pack_coefficients((h.width, h.height), want_p, want_h.quant, (h.hs, h.vs))
        h2.restart_interval = h.restart_interval              # the one field that describes the stream, not the image
        assert bytes(h2) == bytes(h) and torch.equal(buf2, buf), n


def test_entropy_stage_accepts_every_kind_of_buffer(jd, fx):
    data = stream(fx, "s420_40x56")
    h0, b0 = jd.decode_entropy(data)
    for form in (bytearray(data), memoryview(data), np.frombuffer(data, np.uint8), torch.frombuffer(bytearray(data), dtype=torch.uint8)):
        h, b = jd.decode_entropy(form)
        assert bytes(h) == bytes(h0) and torch.equal(b, b0)
    mine = np.full(h0.coeff_bytes + 5, 7, np.uint8)
    h, b = jd.decode_entropy(data, out=mine)
    assert b.numel() == h0.coeff_bytes and torch.equal(b, b0) and (mine[h0.coeff_bytes:] == 7).all()


def test_info_on_every_stream(jd, fx, names):
    for n in names:
        g = fx[f"{n}_geom"]
        info = jd.jpeg_info(stream(fx, n))
        want_s = {(1, 1): "4:4:4", (2, 1): "4:2:2", (2, 2): "4:2:0"}[(int(g[3]), int(g[4]))] if g[2] == 3 else None
        assert info == ((int(g[0]), int(g[1])), "RGB" if g[2] == 3 else "L", want_s, True, None), n
    full = jd.jpeg_info(stream(fx, "full"))
    assert full.size == (1600, 900) and full.sampling == "4:2:0" and full.supported
    prog = jd.jpeg_info(stream(fx, "refused_progressive"))
    assert prog.size == (33, 17) and not prog.supported and "progressive" in prog.reason
    odd = jd.jpeg_info(stream(fx, "refused_1x2"))
    assert odd.size == (33, 17) and not odd.supported and "sampling" in odd.reason
    with pytest.raises(jd.JpegDataError):
        jd.jpeg_info(b"\xff\xd8\xff")
    with pytest.raises(jd.JpegDataError):
        jd.jpeg_info(b"not a jpeg")


def _patched(data, marker, at, value):
    b = bytearray(data)
    b[b.index(marker) + at] = value
    return bytes(b)


def test_refusals_name_their_reason(jd, fx):
    base = stream(fx, "s444_q10")
    cases = {
        "progressive": stream(fx, "refused_progressive"),
        "sampling": stream(fx, "refused_1x2"),
        "8-bit": _patched(base, b"\xff\xc0", 4, 12),
        "components": _patched(_patched(base, b"\xff\xc0", 9, 4), b"\xff\xc0", 3, 20),      # 4 components: the segment is 3 bytes longer
        "arithmetic": _patched(base, b"\xff\xc0", 1, 0xC9),
        "side above": _patched(base, b"\xff\xc0", 7, 0x21),                                   # width 0x2121
    }
    for word, data in cases.items():
        if word == "components":
            data = data[:data.index(b"\xff\xc0") + 19] + b"\x04\x11\x00" + data[data.index(b"\xff\xc0") + 19:]
        info = jd.jpeg_info(data)
        assert not info.supported and word in info.reason, (word, info)
        with pytest.raises(jd.JpegUnsupported, match=word):
            jd.decode_entropy(data)
    # an Adobe segment whose transform flag is not YCbCr, in a stream without a JFIF segment
    at = base.index(b"\xff\xe0")
    n = base[at + 2] << 8 | base[at + 3]
    adobe = lambda t: base[:at] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00" + bytes([t]) + base[at + 2 + n:]
    assert jd.jpeg_info(adobe(1)).supported
    info = jd.jpeg_info(adobe(0))
    assert not info.supported and "YCbCr" in info.reason
    # a scan that holds one of the three components
    sos = base.index(b"\xff\xda")
    one = base[:sos] + b"\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00" + base[sos + 14:]
    assert "scan" in jd.jpeg_info(one).reason


def test_every_proper_prefix_is_refused(jd, fx):
    lib = jd._lib.load()
    for n in PREFIX_CASES:
        data = stream(fx, n)
        h0, want = jd.decode_entropy(data)
        out = np.zeros(h0.coeff_bytes, np.uint8)
        hdr = jd.Header()
        arr = np.frombuffer(data, np.uint8)
        codes = set()
        for k in range(len(data)):
            rc = lib.mopa_jpeg_entropy_decode(arr.ctypes.data, ctypes.addressof(hdr), out.ctypes.data, k, out.size)
            assert rc in (jd.ERR_DATA, jd.ERR_UNSUPPORTED), (n, k, rc)
            codes.add(rc)
        assert codes == {jd.ERR_DATA}, n
        assert lib.mopa_jpeg_entropy_decode(arr.ctypes.data, ctypes.addressof(hdr), out.ctypes.data, len(data), out.size) == 0
        assert np.array_equal(out, want.numpy()), n
    with pytest.raises(jd.JpegDataError):
        jd.decode_entropy(stream(fx, "s420_q10")[:-1])


def test_a_too_small_output_buffer_is_refused(jd, fx):
    lib = jd._lib.load()
    data = stream(fx, "s420_q10")
    arr = np.frombuffer(data, np.uint8)
    hdr = jd.Header()
    assert lib.mopa_jpeg_info(arr.ctypes.data, ctypes.addressof(hdr), arr.size) == 0
    need = lib.mopa_jpeg_coeff_bytes(ctypes.addressof(hdr))
    assert need == hdr.coeff_bytes == 384 + (6 * 4 + 3 * 2 + 3 * 2) * 128
    out = np.full(need, 9, np.uint8)
    assert lib.mopa_jpeg_entropy_decode(arr.ctypes.data, ctypes.addressof(hdr), out.ctypes.data, arr.size, need - 1) == -1
    assert (out == 9).all()                                   # refused before anything is written
    assert lib.mopa_jpeg_entropy_decode(arr.ctypes.data, ctypes.addressof(hdr), None, arr.size, need) == -1
    with pytest.raises(ValueError, match="out holds"):
        jd.decode_entropy(data, out=np.zeros(need - 1, np.uint8))
    # an unsupported stream leaves the buffer alone as well
    bad = np.frombuffer(stream(fx, "refused_progressive"), np.uint8)
    assert lib.mopa_jpeg_entropy_decode(bad.ctypes.data, ctypes.addressof(hdr), out.ctypes.data, bad.size, need) == jd.ERR_UNSUPPORTED
    assert (out == 9).all()
    assert lib.mopa_jpeg_max_images() == 32 and lib.mopa_jpeg_header_bytes() == ctypes.sizeof(jd.Header)
    lib.mopa_jpeg_info(arr.ctypes.data, ctypes.addressof(hdr), arr.size)
    hdr.hs = 3                                                # a header that describes no supported image
    assert lib.mopa_jpeg_coeff_bytes(ctypes.addressof(hdr)) == 0


def test_malformed_streams(jd, fx):
    data = stream(fx, "s444_rst3")
    rst = data.index(b"\xff\xd1")
    sos = data.index(b"\xff\xda") + 14
    bad = {
        "out-of-order restart marker": data[:rst + 1] + b"\xd3" + data[rst + 2:],
        "missing restart marker": data[:rst] + data[rst + 2:],
        "no EOI": data[:-2] + b"\xff\xd8",
        "marker inside a segment": data[:sos + 3] + b"\xff\xd9" + data[sos + 5:],
        "truncated DQT": data[:data.index(b"\xff\xdb") + 2] + b"\xff\xff" + data[data.index(b"\xff\xdb") + 4:],
        "undefined Huffman table": data[:sos - 13] + b"\xff\xda\x00\x0c\x03\x01\x33" + data[sos - 7:],
    }
    for what, d in bad.items():
        with pytest.raises(jd.JpegDataError):
            jd.decode_entropy(d)
        with pytest.raises((ref.DataError, ref.Unsupported)):
            ref.decode_coefficients(d)
    # a Huffman table in which one code is missing: a stream that uses it fails, without reading outside
    dht = data.index(b"\xff\xc4")
    d = bytearray(data)
    d[dht + 5:dht + 21] = bytes(16)                           # no codes at all in the first table
    with pytest.raises(jd.JpegDataError):
        jd.decode_entropy(bytes(d))
    # fill bytes in front of a marker are legal
    filled = data[:rst] + b"\xff\xff\xff" + data[rst:]
    h, b = jd.decode_entropy(filled)
    assert torch.equal(b, jd.decode_entropy(data)[1])
    assert np.array_equal(ref.decode(filled), fx["s444_rst3_rgb"])


# ------------------------------------------------------------------------------------------------ argument checks (no device)
def test_argument_checks_that_need_no_device(jd, fx):
    good = stream(fx, "s420_q10")
    with pytest.raises(TypeError, match="must be bytes"):
        jd.jpeg_info("a string")
    with pytest.raises(TypeError, match="1-D uint8"):
        jd.jpeg_info(np.zeros(4, np.int32))
    with pytest.raises(TypeError, match="1-D uint8"):
        jd.decode_entropy(np.zeros((2, 2), np.uint8))
    with pytest.raises(TypeError, match="1-D uint8"):
        jd.decode_entropy(torch.zeros(4, dtype=torch.int16))
    with pytest.raises(ValueError, match="out must be a contiguous 1-D uint8"):
        jd.decode_entropy(good, out=torch.zeros(4000, dtype=torch.int16))
    with pytest.raises(TypeError, match="list of streams"):
        jd.decode_jpeg_batch(good)
    with pytest.raises(ValueError, match="no streams"):
        jd.decode_jpeg_batch([])
    with pytest.raises(TypeError, match=r"datas\[1\]"):
        jd.decode_jpeg_batch([good, 5])
    with pytest.raises(ValueError, match="threads"):
        jd.decode_jpeg_batch([good], threads=0)
    with pytest.raises(jd.JpegUnsupported, match=r"datas\[1\]: unsupported stream: progressive"):
        jd.decode_jpeg_batch([good, stream(fx, "refused_progressive")])
    with pytest.raises(jd.JpegDataError, match=r"datas\[0\]"):
        jd.decode_jpeg_batch([good[:40], good])
    assert issubclass(jd.JpegUnsupported, ValueError) and issubclass(jd.JpegDataError, ValueError)
    # out: count, type, dtype, shape, strides come before the device
    host = torch.zeros(17, 33, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="list of 1 tensors"):
        jd.decode_jpeg_batch([good], out=[host, host])
    with pytest.raises(TypeError, match="torch tensor"):
        jd.decode_jpeg_batch([good], out=[np.zeros((17, 33, 3), np.uint8)])
    with pytest.raises(TypeError, match="uint8"):
        jd.decode_jpeg_batch([good], out=[host.float()])
    with pytest.raises(ValueError, match=r"must be \(17, 33, 3\)"):
        jd.decode_jpeg_batch([good], out=[torch.zeros(33, 17, 3, dtype=torch.uint8)])
    with pytest.raises(ValueError, match="strides"):
        jd.decode_jpeg_batch([good], out=[torch.zeros(17, 3, 33, dtype=torch.uint8).permute(0, 2, 1)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        jd.decode_jpeg_batch([good], out=[host])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        jd.decode_jpeg_batch([good], device="cpu")
    # the device half's own checks
    h, b = jd.decode_entropy(good)
    with pytest.raises(ValueError, match="one buffer per header"):
        jd.decode_coefficients_batch([h], [])
    with pytest.raises(TypeError, match="jpegdec.Header"):
        jd.decode_coefficients_batch([object()], [b])
    with pytest.raises(TypeError, match="1-D uint8"):
        jd.decode_coefficients_batch([h], [b.view(torch.int16)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        jd.decode_coefficients_batch([h], [b], device="cpu")
    with pytest.raises(ValueError, match="not a supported image"):
        jd.pack_coefficients((33, 17), [np.zeros((3, 5, 64), np.int16)] * 2, np.ones((2, 64), np.uint16))
    with pytest.raises(ValueError, match="plane 0"):
        jd.pack_coefficients((33, 17), [np.zeros((3, 4, 64), np.int16)], np.ones((1, 64), np.uint16))


def test_out_overlap_is_found_on_strided_views(jd):
    a = torch.zeros(20, 40, 3, dtype=torch.uint8)
    assert jd._overlap(a[:10], a[5:]) and not jd._overlap(a[:10], a[10:])
    assert jd._overlap(a[:, :10], a[:, 10:20])                # interleaved column windows share the span


# ------------------------------------------------------------------------------------------------ the sanitizer program
def test_entropy_stage_under_the_sanitizers(fx, tmp_path):
    """tests/jpeg_entropy_check.cpp, compiled with the host compiler under -fsanitize=address,undefined, over every prefix of three
    small streams and a fixed set of single-byte substitutions (about 3300 streams): it must exit 0 and report nothing."""
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "clang++", "c++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "jpeg_entropy_check"
    src = os.path.join(ROOT, "tests", "jpeg_entropy_check.cpp")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    # the runtimes linked statically where the compiler can (g++'s spelling): the program then depends on nothing around it
    for extra in (["-static-libasan", "-static-libubsan"], []):
        build = subprocess.run([cxx] + flags + extra + [src, "-o", str(exe)], capture_output=True, text=True)
        if build.returncode == 0:
            break
    if build.returncode != 0 and "cannot find" in build.stderr and "san" in build.stderr:
        pytest.skip("the host compiler has no sanitizer runtime")
    assert build.returncode == 0, build.stderr
    files = []

    def put(name, data):
        p = tmp_path / name
        p.write_bytes(data)
        files.append(str(p))

    rng = np.random.Generator(np.random.PCG64(2016))
    for n in PREFIX_CASES:
        data = stream(fx, n)
        put(f"{n}_good", data)
        for k in range(len(data)):
            put(f"{n}_p{k}_bad", data[:k])
        # substitutions: every byte of the headers gets 0x00 / 0xFF / a draw in turn, the entropy-coded bytes a draw each 3rd byte
        sos = data.index(b"\xff\xda")
        for k in range(2, len(data)):
            if k > sos + 14 and k % 3:
                continue
            v = (0x00, 0xFF, int(rng.integers(0, 256)))[k % 3]
            if v != data[k]:
                put(f"{n}_s{k}", data[:k] + bytes([v]) + data[k + 1:])
    for n in ("refused_progressive", "refused_1x2", "grey_33x17", "s420_rst1", "s422_opt", "s444_q100"):
        put(f"{n}_any", stream(fx, n))
    assert 1000 < len(files) < 6000
    run = subprocess.run([str(exe)] + files, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert run.stderr == "" and run.stdout.strip().endswith("0 failures"), (run.stdout[-500:], run.stderr[-2000:])
