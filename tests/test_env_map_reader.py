"""The environment-map readers of the host (EnvMapReader: Radiance .hdr flat and RLE, .pfm of both byte orders, .exr) through the
test shim's pth_read_env_map, and every truncation of every file under AddressSanitizer + UBSan.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ipu_path_trace_amd", "host")
SIZES = ((8, 4), (40, 3))   # W x H


@pytest.fixture(scope="module")
def host():
    subprocess.check_call(["make", "-C", HOST, "-s"])
    L = C.CDLL(os.path.join(HOST, "libpthost.so"))
    L.pth_read_env_map.argtypes = [C.c_char_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.c_char_p,
                                   C.c_size_t]
    L.pth_write_exr.argtypes = [C.c_char_p, C.c_void_p, C.c_size_t, C.c_size_t]
    L.pth_write_exr.restype = None
    return L


def _read(host, path, capacity=1 << 16):
    out = np.zeros(capacity, dtype=np.float32)
    w, h = C.c_size_t(), C.c_size_t()
    err = C.create_string_buffer(1024)
    rc = host.pth_read_env_map(str(path).encode(), out.ctypes.data, out.size, C.byref(w), C.byref(h), err, len(err))
    if rc:
        return rc, err.value.decode()
    return 0, out[:3 * w.value * h.value].reshape(h.value, w.value, 3).copy()


def _rgbe(W, H, seed):
    """Random RGBE pixels [H, W, 4] with runs along the rows (so the RLE writer emits both packet kinds) and a black pixel."""
    rng = np.random.default_rng(seed)
    px = rng.integers(0, 256, (H, W, 4)).astype(np.uint8)
    px[..., 3] = rng.integers(120, 141, (H, W))
    px[:, 2:6] = px[:, 2:3]                 # a run of four equal pixels in every row
    if W > 20:
        px[:, 10:, 3] = 130                 # a long run in the exponent plane
    px[0, 1] = (17, 99, 201, 0)             # exponent 0: black, whatever the mantissas
    return px


def _decode(px):
    """The test's own decode: mantissa * 2^(e - 136), 0 for e == 0, as BGR rows top to bottom."""
    e = px[..., 3].astype(np.int64)
    scale = np.where(e == 0, 0.0, np.ldexp(1.0, e - 136))
    rgb = px[..., :3].astype(np.float64) * scale[..., None]
    return rgb[..., ::-1].astype(np.float32)


def _rle_channel(row):
    out, i, n = bytearray(), 0, len(row)
    while i < n:
        run = 1
        while i + run < n and run < 127 and row[i + run] == row[i]:
            run += 1
        if run >= 3:
            out += bytes([128 + run, row[i]])
            i += run
            continue
        j = i
        while j < n and j - i < 128:
            if j + 2 < n and row[j] == row[j + 1] == row[j + 2]:
                break
            j += 1
        out += bytes([j - i]) + bytes(row[i:j])
        i = j
    return bytes(out)


def _write_hdr(path, px, rle, magic=b"#?RADIANCE", res=None):
    H, W, _ = px.shape
    body = bytearray()
    for y in range(H):
        if rle:
            body += bytes([2, 2, W >> 8, W & 255])
            for c in range(4):
                body += _rle_channel([int(x) for x in px[y, :, c]])
        else:
            body += px[y].tobytes()
    with open(path, "wb") as f:
        f.write(magic + b"\n# written by the test\nFORMAT=32-bit_rle_rgbe\nEXPOSURE=1.0\n\n")
        f.write(res if res is not None else b"-Y %d +X %d\n" % (H, W))
        f.write(bytes(body))


def _write_pfm(path, bgr, little):
    H, W, _ = bgr.shape
    with open(path, "wb") as f:
        f.write(b"PF\n%d %d\n%s\n" % (W, H, b"-1.0" if little else b"1.0"))
        f.write(np.ascontiguousarray(bgr[::-1, :, ::-1], dtype="<f4" if little else ">f4").tobytes())


def _float_image(W, H, seed):
    return np.random.default_rng(seed).uniform(0.0, 50.0, (H, W, 3)).astype(np.float32)


def _all_files(host, tmp_path):
    """(path, expected BGR) of every file the tests read."""
    files = []
    for W, H in SIZES:
        px = _rgbe(W, H, 10 * W + H)
        for rle in (False, True):
            p = tmp_path / ("%s_%dx%d.hdr" % ("rle" if rle else "flat", W, H))
            _write_hdr(str(p), px, rle, magic=b"#?RGBE" if rle else b"#?RADIANCE")
            files.append((p, _decode(px)))
        img = _float_image(W, H, W)
        for little in (True, False):
            p = tmp_path / ("%s_%dx%d.pfm" % ("le" if little else "be", W, H))
            _write_pfm(str(p), img, little)
            files.append((p, img))
        p = tmp_path / ("img_%dx%d.exr" % (W, H))
        host.pth_write_exr(str(p).encode(), img.ctypes.data, W, H)
        files.append((p, img))
    return files


def _packet_kinds(enc):
    kinds, i = set(), 0
    while i < len(enc):
        if enc[i] > 128:
            kinds.add("run")
            i += 2
        else:
            kinds.add("literal")
            i += 1 + enc[i]
    return kinds


def test_every_format_reads_back_exactly(host, tmp_path):
    # the fixture first: the RLE writer really emits both packet kinds, and its files differ from the flat ones
    px = _rgbe(40, 3, 10 * 40 + 3)
    for c in (0, 3):
        assert _packet_kinds(_rle_channel([int(x) for x in px[1, :, c]])) == {"run", "literal"}
    files = _all_files(host, tmp_path)
    assert (tmp_path / "flat_40x3.hdr").read_bytes()[10:] != (tmp_path / "rle_40x3.hdr").read_bytes()[6:]
    for path, want in files:
        rc, got = _read(host, path)
        assert rc == 0, got
        assert got.shape == want.shape, path
        assert got.tobytes() == want.tobytes(), path          # RGBE exact after mantissa * 2^(e - 136); floats bit for bit


def test_rows_are_top_to_bottom(host, tmp_path):
    W, H = 8, 4
    rows = np.zeros((H, W, 3), dtype=np.float32)
    rows[...] = np.arange(H, dtype=np.float32)[:, None, None] + 1.0       # row r holds r + 1
    rows[..., 1] *= 2                                                     # G = 2 (r + 1), R = 3 (r + 1)
    rows[..., 2] *= 3
    _write_pfm(str(tmp_path / "rows.pfm"), rows, True)
    host.pth_write_exr(str(tmp_path / "rows.exr").encode(), rows.ctypes.data, W, H)
    px = np.zeros((H, W, 4), dtype=np.uint8)
    px[..., 3] = 136                                                      # value == mantissa
    for r in range(H):
        px[r, :, :3] = (3 * (r + 1), 2 * (r + 1), r + 1)                  # R, G, B in the file
    _write_hdr(str(tmp_path / "rows.hdr"), px, False)
    for name in ("rows.pfm", "rows.exr", "rows.hdr"):
        rc, got = _read(host, tmp_path / name)
        assert rc == 0, got
        assert np.array_equal(got, rows), name


def test_refusals_name_the_reason(host, tmp_path):
    px = _rgbe(8, 4, 3)
    for res in (b"+Y 4 +X 8\n", b"-Y 4 -X 8\n", b"+X 8 -Y 4\n"):
        _write_hdr(str(tmp_path / "o.hdr"), px, False, res=res)
        rc, msg = _read(host, tmp_path / "o.hdr")
        assert rc == -1 and res.strip().decode() in msg and "orientation" in msg
    (tmp_path / "x.hdr").write_bytes(b"#?RADIANCE\nFORMAT=32-bit_rle_xyze\n\n-Y 4 +X 8\n" + bytes(128))
    rc, msg = _read(host, tmp_path / "x.hdr")
    assert rc == -1 and "32-bit_rle_xyze" in msg
    (tmp_path / "g.pfm").write_bytes(b"Pf\n2 2\n-1.0\n" + bytes(16))
    rc, msg = _read(host, tmp_path / "g.pfm")
    assert rc == -1 and "Pf" in msg
    (tmp_path / "big.pfm").write_bytes(b"PF\n20000 2\n-1.0\n" + bytes(16))
    rc, msg = _read(host, tmp_path / "big.pfm")
    assert rc == -1 and "16384" in msg
    rc, msg = _read(host, tmp_path / "missing.hdr")
    assert rc == -1 and "missing.hdr" in msg
    _write_pfm(str(tmp_path / "ok.pfm"), _float_image(8, 4, 0), True)
    assert _read(host, tmp_path / "ok.pfm", capacity=10)[0] == -2


def test_every_truncation_fails_cleanly_under_the_sanitizers(host, tmp_path):
    """Every proper prefix of every file must end in an exception that names the file and an offset.  The reader is built with
    AddressSanitizer + UBSan here, so an out-of-bounds read that happens not to crash is caught as well."""
    exe = str(tmp_path / "envmap_fuzz")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + HOST, "-o", exe, os.path.join(ROOT, "tests", "envmap_fuzz_main.cpp"),
                           os.path.join(HOST, "EnvMapReader.cpp")])
    files = [str(p) for p, _ in _all_files(host, tmp_path)]
    total = sum(os.path.getsize(f) for f in files)
    cuts = tmp_path / "cuts"
    cuts.mkdir()
    r = subprocess.run([exe, str(cuts)] + files, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:allocator_may_return_null=1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    whole, rejected, accepted, unnamed = [int(x) for x in r.stdout.strip().splitlines()[-1].split()[1::2]]
    assert whole == len(files) == 10, r.stdout[-2000:]
    assert accepted == 0 and unnamed == 0, r.stdout[-2000:]
    assert rejected == total
