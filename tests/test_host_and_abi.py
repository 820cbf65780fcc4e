"""CPU tests of the host side and the C-ABI surface: RNG / sincos definitions, film, PPM, PNG, the exported symbols
of include/*.h, and the "no GPU -> fail loudly" behaviour. No compute entry point is called without a GPU."""
import ctypes
import os
import re
import struct
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


# ------------------------------------------------------------------------------------------------ ABI surface
def _declared_functions(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol(rt):
    lib = rt.lib()
    names = _declared_functions("rt_abi.h") + _declared_functions("rt_host.h")
    assert "rt_render" in names and "rt_create" in names and "rt_gltf_load" in names
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/ but not exported by librt_amd.so"
    assert lib.rt_abi_version() == 4


def test_ctypes_prototypes_cover_the_headers(rt):
    abi = __import__("importlib").import_module("raytracing-course-hw-public_amd._ctypes_abi")
    declared = set(_declared_functions("rt_abi.h")) | set(_declared_functions("rt_host.h"))
    bound = set(abi.ABI_PROTOTYPES) | set(abi.HOST_PROTOTYPES)
    assert declared == bound, declared ^ bound


def _abi():
    return __import__("importlib").import_module("raytracing-course-hw-public_amd._ctypes_abi")


def _compile_and_run(tmp_path, name, body):
    """The whitespace-separated integers a C program prints whose main() is `body`, compiled against include/rt_abi.h."""
    import subprocess

    src = tmp_path / (name + ".c")
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_abi.h"\nint main(void){\n' + body + "return 0;}\n")
    exe = tmp_path / name
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    return [int(x) for x in subprocess.check_output([str(exe)]).split()]


def test_struct_layouts_match_the_c_headers(rt, tmp_path):
    """sizeof of every struct and offsetof of every field as the C compiler sees them == the ctypes mirrors: every ctypes.Structure of
    _ctypes_abi has exactly one typedef of rt_abi.h (its name in snake_case, or that + _desc), and no struct of the header lacks a mirror."""
    abi = _abi()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rt_abi.h")).read(), flags=re.S)
    typedefs = set(re.findall(r"typedef\s+struct\s+(rt_\w+)\s*\{", header))
    mirrors = {}
    for cls in vars(abi).values():
        if isinstance(cls, type) and issubclass(cls, ctypes.Structure) and cls is not ctypes.Structure:
            snake = re.sub(r"(?<!^)(?=[A-Z])", "_", cls.__name__).lower()
            match = {snake, snake + "_desc"} & typedefs
            assert len(match) == 1, f"{cls.__name__}: {sorted(match)} of rt_abi.h match"
            mirrors[match.pop()] = cls
    assert set(mirrors) == typedefs, f"no ctypes mirror: {sorted(typedefs - set(mirrors))}"
    exprs, want = [], []
    for cname, cls in sorted(mirrors.items()):
        exprs.append(f"sizeof({cname})")
        want.append(ctypes.sizeof(cls))
        for field, _ in cls._fields_:
            exprs.append(f"offsetof({cname}, {field})")
            want.append(getattr(cls, field).offset)
    got = _compile_and_run(tmp_path, "layouts", "".join(f'printf("%zu\\n", {e});\n' for e in exprs))
    assert len(mirrors) >= 21 and len(want) >= 182
    wrong = [(e, g, w) for e, g, w in zip(exprs, got, want) if g != w]
    assert len(got) == len(want) and not wrong, wrong


def test_constants_match_the_c_headers(rt, tmp_path):
    """Every RT_* integer of _ctypes_abi and every name of ERROR_NAMES has the value rt_abi.h gives it (a name the header lacks does not
    compile)."""
    abi = _abi()
    want = {n: v for n, v in vars(abi).items() if re.fullmatch(r"RT_[A-Z0-9_]+", n) and isinstance(v, int) and not isinstance(v, bool)}
    assert want["RT_ALL_DEVICES"] == -1 and want["RT_SENSOR_THIN_LENS"] == 4 and len(want) >= 50
    want.update({name: code for code, name in abi.ERROR_NAMES.items()})
    names = sorted(want)
    got = _compile_and_run(tmp_path, "constants", "".join(f'printf("%lld\\n", (long long)({n}));\n' for n in names))
    wrong = [(n, g, want[n]) for n, g in zip(names, got) if g != want[n]]
    assert len(got) == len(names) and not wrong, wrong


def test_library_reads_no_environment_variable():
    """ABI 4: every knob is a field of rt_scene_desc / rt_params (the reference's are constexpr, config.h:7-47). getenv appears
    only in the CLI (csrc/host/main.cpp), which translates variables into fields; bench.py does the same on the Python side."""
    csrc = os.path.join(ROOT, "raytracing-course-hw-public_amd", "csrc")
    hits = []
    for d, _, files in os.walk(csrc):
        for f in files:
            if f.endswith((".cpp", ".hip", ".h")) and not (d.endswith("host") and f == "main.cpp"):
                text = open(os.path.join(d, f)).read()
                if re.search(r"\bgetenv\b|\bsecure_getenv\b|\benviron\b", text):
                    hits.append(os.path.relpath(os.path.join(d, f), csrc))
    assert hits == [], hits


def test_sub_queue_regions_tile_the_queue(tmp_path):
    """wf_shade's 64 output sub-queues (rt_device_types.h, wf_stripe_base): for any number of wave slots the regions are
    disjoint, in order, each exactly as large as the slots dealt to it round-robin (so a region can never overflow), and
    together they cover [0, 64 * slots)."""
    import subprocess

    src = tmp_path / "stripes.cpp"
    src.write_text(
        '#include <cstdio>\n#include "rt_device_types.h"\n'
        "int main(){ const unsigned K = WF_STRIPES; unsigned long long bad = 0;\n"
        " const unsigned cases[] = {0,1,2,63,64,65,127,128,129,1000,4095,4096,4097,65535,1000003,1048576};\n"
        " for (unsigned n : cases) { unsigned expect = 0;\n"
        "  for (unsigned k = 0; k < K; ++k) { const unsigned slots_k = n / K + (k < n % K ? 1u : 0u);\n"
        "   if (wf_stripe_base(k, n) != expect) ++bad; expect += 64u * slots_k; }\n"
        "  if (expect != 64u * n) ++bad; }\n"
        ' printf("%llu %u %u\\n", bad, (unsigned)WF_STRIPES, (unsigned)WF_STRIPE_BUF_WORDS); return 0; }\n'
    )
    exe = tmp_path / "stripes"
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "raytracing-course-hw-public_amd", "csrc"), str(src), "-o", str(exe)])
    bad, k, words = (int(x) for x in subprocess.check_output([str(exe)]).split())
    assert bad == 0 and k == 64 and words == 64 * 32 + 65


def test_no_gpu_fails_loudly(rt, sg):
    """The product never falls back to a CPU path: without a HIP device rt_create reports RT_ERR_NO_DEVICE. Its argument checks come
    first, on every machine: a non-zero reserved rt_build_options field or an undefined build_flags bit (8 was a development flag)
    is RT_ERR_INVALID_ARG before any device is looked for."""
    sc = sg.boxes_scene(n_boxes=1, seed=1)
    for bad in ({"reserved0": 1}, {"reserved1": 1}, {"reserved": 1}, {"build_flags": 8}, {"build_flags": 64}):
        with pytest.raises(rt.RtError) as e:
            rt.DeviceScene(sc, **bad)
        assert e.value.code == 1, bad
    if rt.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(rt.RtError) as e:
        rt.DeviceScene(sc)
    assert e.value.code == 2 and "no CPU fallback" in str(e.value)


def test_product_does_not_reference_the_oracle():
    """Only tests/, bench.py's cpu_baseline leg and __graft_entry__.smoke() may touch oracle/."""
    pkg = os.path.join(ROOT, "raytracing-course-hw-public_amd")
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h", "Makefile")):
                text = open(os.path.join(d, f), errors="ignore").read()
                assert "liboracle" not in text and "rto_" not in text and "rt_oracle" not in text, f


# ------------------------------------------------------------------------------------------------ RNG / sincos
def test_minstd_distributions_match_libstdcxx(oracle):
    """include/rt_devspec.h rt_minstd_* == std::minstd_rand + uniform_real<float> / uniform_int<> of libstdc++ 11."""
    kat = np.load(os.path.join(GOLD, "rng_kat.npz"))
    for seed in (0, 1, 2, 42, 3906):
        got = oracle.minstd_sequence(seed, 64)
        assert np.array_equal(got.view(np.uint32), kat[f"real_{seed}"].view(np.uint32)), seed
        for bound in (1, 2, 3, 16, 1000):
            assert np.array_equal(oracle.minstd_below_sequence(seed, bound, 64), kat[f"int_{seed}_{bound}"]), (seed, bound)
    # seeds 0 and 1 share a stream
    assert np.array_equal(kat["real_0"], kat["real_1"])
    # uniform_real(-1, 1) = canonical * 2 - 1
    c = oracle.minstd_sequence(7, 64)
    assert np.array_equal((c * np.float32(2.0) + np.float32(-1.0)).view(np.uint32), kat["range_7_m1_1"].view(np.uint32))


def test_xoshiro_streams(oracle):
    a = oracle.xoshiro_sequence(123, 5, 0, 4096)
    b = oracle.xoshiro_sequence(123, 5, 1, 4096)
    c = oracle.xoshiro_sequence(123, 6, 0, 4096)
    assert (a >= 0).all() and (a < 1).all()
    assert abs(a.mean() - 0.5) < 0.02 and abs(a.var() - 1 / 12) < 0.01
    assert not np.array_equal(a, b) and not np.array_equal(a, c)
    assert np.array_equal(a, oracle.xoshiro_sequence(123, 5, 0, 4096))
    assert np.all(a * np.float32(2**24) == np.floor(a * np.float32(2**24)))  # exact multiples of 2^-24


def test_xoshiro_against_published_vectors_and_an_independent_restatement(oracle):
    """include/rt_devspec.h's xoshiro128++ is compiled into BOTH the kernels and the oracle, so "GPU == oracle" cannot tell whether it is
    the published generator. Pinned here from outside: (a) the engine against the known answers of Blackman & Vigna's xoshiro128++ for the
    state {1, 2, 3, 4} (the vector the public implementations test with), (b) seeding (splitmix64 of seed ^ (pixel, sample) * odd constant),
    the 24-bit canonical float and the multiply-shift bounded integer against a restatement in plain Python integers."""
    published = [641, 1573767, 3222811527, 3517856514, 836907274, 4247214768, 3867114732, 1355841295, 495546011, 621204420]
    assert oracle.xoshiro_raw([1, 2, 3, 4], 10).tolist() == published
    M32, M64 = (1 << 32) - 1, (1 << 64) - 1

    def splitmix(x):
        x = (x + 0x9E3779B97F4A7C15) & M64
        z = x
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        return x, z ^ (z >> 31)

    def rotl(v, k):
        return ((v << k) | (v >> (32 - k))) & M32

    def stream(seed, pixel, sample, n):
        x = (seed ^ ((((pixel << 32) | sample) * 0xD1342543DE82EF95) & M64)) & M64
        x, a = splitmix(x)
        x, b = splitmix(x)
        s = [a & M32, a >> 32, b & M32, b >> 32]
        if not any(s):
            s[0] = 1
        out = []
        for _ in range(n):
            out.append((rotl((s[0] + s[3]) & M32, 7) + s[0]) & M32)
            t = (s[1] << 9) & M32
            s[2] ^= s[0]
            s[3] ^= s[1]
            s[1] ^= s[2]
            s[0] ^= s[3]
            s[2] ^= t
            s[3] = rotl(s[3], 11)
        return out

    assert splitmix(1234567)[1] == 6457827717110365317  # splitmix64's published first output for this seed
    for seed, pixel, sample in ((0, 0, 0), (1, 0, 0), (0xDEADBEEFCAFEF00D, 999999, 63), (7, 0xFFFFFFFF, 0xFFFFFFFF), (2**64 - 1, 123456, 999)):
        raw = stream(seed, pixel, sample, 256)
        got = oracle.xoshiro_sequence(seed, pixel, sample, 256)
        want = np.array([(r >> 8) for r in raw], dtype=np.float64) * 2.0**-24
        assert np.array_equal(got.astype(np.float64), want), (seed, pixel, sample)
        for bound in (1, 2, 16, 40, 1000, 2**31 + 5):
            assert oracle.xoshiro_below_sequence(seed, pixel, sample, bound, 256).tolist() == [(r * bound) >> 32 for r in raw], bound


def test_sincos_restatement_against_libm_and_float64(oracle):
    """rt_sincos_libm (what the device evaluates) against the host libm the oracle calls — bit-identical on a sample (the exhaustive comparison
    over all of [0, 2*pi] is test_libm_sincos_restatement_is_exhaustively_glibc) — and against float64: glibc's documented < 0.56 ulp."""
    rng = np.random.default_rng(1)
    phi = np.concatenate([rng.uniform(0, 2 * np.pi, 200000), [0.0, np.pi / 2, np.pi, 1.5 * np.pi, 2 * np.pi], np.linspace(0, 2 * np.pi, 4097)]).astype(np.float32)
    s, c = oracle.sincos(phi)
    ls, lc = oracle.sincos(phi, libm=True)
    assert np.array_equal(s.view(np.uint32), ls.view(np.uint32)) and np.array_equal(c.view(np.uint32), lc.view(np.uint32))
    for got, true in ((s, np.sin(phi.astype(np.float64))), (c, np.cos(phi.astype(np.float64)))):
        ulp = np.spacing(np.abs(true).astype(np.float32)).astype(np.float64)
        err = np.abs(got.astype(np.float64) - true) / np.maximum(ulp, 1e-45)
        assert err.max() <= 0.56, err.max()
    assert np.all(s * s + c * c < 1.0000003)


def test_one_step_exact_division_hard_cases(tmp_path):
    """The slab test's 3-op exact division (div_exact_fast: a*r, one FMA residual, one FMA correction) equals IEEE
    division on every significand pair that comes close enough to a rounding boundary to be at risk (exhaustive
    enumeration, tools/proofs/div_one_step.c) — the argument that lets the HIP path drop the second correction."""
    import subprocess

    exe = str(tmp_path / "div_one_step")
    subprocess.check_call(["gcc", "-O2", os.path.join(ROOT, "tools", "proofs", "div_one_step.c"), "-o", exe, "-lm"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert ", failures 0 " in r.stdout and "random failures 0" in r.stdout


def test_libm_sincos_restatement_is_exhaustively_glibc(tmp_path):
    """rt_sincos_libm (include/rt_devspec.h), which the device evaluates in reference-RNG mode where the reference calls
    std::sin / std::cos (raytracer.h:104,158-159), equals the host's glibc sinf / cosf on EVERY float in [0, 2*pi]
    (1.09e9 values, tools/proofs/sincosf_exhaustive.c) — the last link of "GPU image = the reference binary's image"."""
    import subprocess

    exe = str(tmp_path / "sincosf_exhaustive")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tools", "proofs", "sincosf_exhaustive.c"), "-o", exe, "-lm", "-lpthread"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "mismatches against libm sinf/cosf: 0 " in r.stdout


# ------------------------------------------------------------------------------------------------ film / PPM / PNG
def test_tonemap_matches_oracle_film(rt, oracle):
    rng = np.random.default_rng(3)
    fb = np.concatenate([rng.uniform(0, 4, 30000), rng.uniform(0, 0.01, 3000), [0.0, 1.0, 1e6, 0.18]]).astype(np.float32)
    fb = fb[: (fb.size // 3) * 3].reshape(-1, 1, 3)
    a, b = rt.tonemap(fb), oracle.tonemap(fb)
    assert np.array_equal(a, b)
    assert a.min() == 0 and a.max() == 255


def test_film_threshold_table_reproduces_the_host_film(rt, oracle):
    """The device film's gamma stage (rt_film_table: 255 thresholds over the ACES value, built from libm powf) gives the
    same level as the host film and the oracle film for random radiances over all exponents; numpy float32 ACES is the
    same five IEEE operations."""
    thr, special = rt.film_table()
    assert thr[0] == 0 and np.all(np.diff(thr) > 0) and thr[255] < 1.0
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.uniform(0, 4, 600000), 10.0 ** rng.uniform(-44, 38, 100000), [0.0, 1e-45, 3e38, np.inf, 0.18]]).astype(np.float32)
    x = x[: (x.size // 3) * 3]
    a, b, c, d, e = (np.float32(v) for v in (2.51, 0.03, 2.43, 0.59, 0.14))
    with np.errstate(all="ignore"):
        y = (x * (a * x + b)) / (x * (c * x + d) + e)
    lvl = np.where(np.isnan(y), special[0], np.searchsorted(thr, y, side="right") - 1).astype(np.uint8)
    want = oracle.tonemap(x.reshape(-1, 1, 3)).reshape(-1)
    assert np.array_equal(lvl, want)
    assert np.array_equal(rt.tonemap(x.reshape(-1, 1, 3)).reshape(-1), want)
    neg = oracle.tonemap(np.array([[[-0.001, -np.inf, np.nan]]], dtype=np.float32)).reshape(-1)
    # ACES of -0.001 is negative finite, of -inf and NaN is NaN: the documented specials
    assert int(neg[0]) == int(special[1]) and int(neg[1]) == int(special[0]) and int(neg[2]) == int(special[0])


def test_ppm_roundtrip_and_directory_creation(rt, oracle, tmp_path):
    img = np.random.default_rng(4).integers(0, 256, size=(7, 5, 3), dtype=np.uint8)
    path = tmp_path / "deep" / "er" / "o.ppm"  # main.cpp:41 create_directories
    rt.write_ppm(str(path), img)
    data = path.read_bytes()
    assert data.startswith(b"P6\n5 7\n255\n") and len(data) == 11 + 5 * 7 * 3
    assert np.array_equal(oracle.read_ppm(str(path)), img)


def _png(path, img, filters):
    h, w, c = img.shape
    ctype = {1: 0, 2: 4, 3: 2, 4: 6}[c]
    raw = bytearray()
    prev = np.zeros((w, c), dtype=np.int32)
    for y in range(h):
        row = img[y].astype(np.int32)
        ft = filters[y % len(filters)]
        left = np.vstack([np.zeros((1, c), np.int32), row[:-1]])
        upleft = np.vstack([np.zeros((1, c), np.int32), prev[:-1]])
        if ft == 0:
            enc = row
        elif ft == 1:
            enc = row - left
        elif ft == 2:
            enc = row - prev
        elif ft == 3:
            enc = row - ((left + prev) >> 1)
        else:
            p = left + prev - upleft
            pa, pb, pc = np.abs(p - left), np.abs(p - prev), np.abs(p - upleft)
            pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, prev, upleft))
            enc = row - pred
        raw += bytes([ft]) + (enc & 255).astype(np.uint8).tobytes()
        prev = row

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    comp = zlib.compress(bytes(raw))
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, ctype, 0, 0, 0)))
        f.write(chunk(b"IDAT", comp[: len(comp) // 2]) + chunk(b"IDAT", comp[len(comp) // 2 :]) + chunk(b"IEND", b""))


@pytest.mark.parametrize("channels", [1, 2, 3, 4])
def test_png_decoder_all_filters_and_colour_types(rt, tmp_path, channels):
    img = np.random.default_rng(channels).integers(0, 256, size=(13, 9, channels), dtype=np.uint8)
    p = str(tmp_path / f"t{channels}.png")
    _png(p, img, filters=[0, 1, 2, 3, 4])
    out = rt.png_decode(p)
    assert out.shape == (13, 9, 4)
    if channels == 1:
        want = np.concatenate([img, img, img, np.full_like(img, 255)], axis=2)
    elif channels == 2:
        want = np.concatenate([img[..., :1]] * 3 + [img[..., 1:]], axis=2)
    elif channels == 3:
        want = np.concatenate([img, np.full((13, 9, 1), 255, np.uint8)], axis=2)
    else:
        want = img
    assert np.array_equal(out, want)


def test_loader_errors_are_codes_not_crashes(rt, tmp_path):
    with pytest.raises(rt.RtError):
        rt.parse_gltf_scene(str(tmp_path / "missing.gltf"), 1.0)
    bad = tmp_path / "bad.gltf"
    bad.write_text('{"scenes":[{"nodes":[0]}],"nodes":[{"mesh":0}],"meshes":[{"primitives":[{"attributes":{"POSITION":0}}]}],"buffers":[],"accessors":[]}')
    with pytest.raises(rt.RtError) as e:
        rt.parse_gltf_scene(str(bad), 1.0)
    assert "material" in str(e.value)
    with pytest.raises(rt.RtError):
        rt.png_decode(str(bad))


def test_png_decoder_rejects_malformed_headers(rt, tmp_path):
    """Untrusted IHDR fields: dimensions whose byte count would wrap size_t, zero sizes, truncated streams, bad filter
    bytes and short IDAT data must come back as RT_ERR_FORMAT, never as an out-of-bounds access."""

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    def png(w, h, depth=8, ctype=6, interlace=0, raw=b"\x00" * 64, cut=None):
        blob = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, interlace)) + chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b"")
        return blob if cut is None else blob[:cut]

    cases = {
        "huge_w": png(0xFFFFFFFF, 2),
        "huge_h": png(2, 0xFFFFFFFF),
        "wrap": png(0x40000001, 0x40000001),  # (stride + 1) * h wraps 64-bit size_t with 4 channels
        "big_product": png(1 << 20, 1 << 20),
        "zero_w": png(0, 4),
        "short_idat": png(4, 4, raw=b"\x00" * 10),
        "bad_filter": png(2, 2, raw=b"\x07" + b"\x00" * 8 + b"\x00" + b"\x00" * 8),
        "bad_ctype": png(2, 2, ctype=5),
        "truncated": png(4, 4, raw=b"\x00" * 68, cut=40),
        "not_png": b"JFIF" * 20,
    }
    for name, blob in cases.items():
        p = tmp_path / (name + ".png")
        p.write_bytes(blob)
        with pytest.raises(rt.RtError) as e:
            rt.png_decode(str(p))
        assert e.value.code == 6, name  # RT_ERR_FORMAT


# ------------------------------------------------------------------------------------------------ INTEGRATION.md binding
REFERENCE_SRC = "/root/reference/src"


@pytest.mark.skipif(not os.path.isdir(REFERENCE_SRC), reason="needs the reference headers (absent on the GPU box)")
def test_integration_binding_compiles_against_the_reference(tmp_path):
    """The C++ binding INTEGRATION.md tells a maintainer to add (run_raytracer_amd in place of run_raytracer,
    src/main.cpp:37) must keep compiling against the reference's own headers (scene.h:74-90, geometry.h:633-643,
    image.h:14-83) and include/rt_abi.h: every ```cpp block of the file is extracted and syntax-checked, the two
    statement-level snippets inside a function body."""
    import subprocess

    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    blocks = re.findall(r"```cpp\n(.*?)```", text, flags=re.S)
    binding = [b for b in blocks if "run_raytracer_amd" in b and "#include" in b]
    assert len(binding) == 1, "INTEGRATION.md must hold exactly one complete binding block"
    src = tmp_path / "binding_check.cpp"
    parts = ["#include <cmath>\n#include <vector>\n", binding[0]]
    # the rgb8 variant: statements that live inside run_raytracer_amd, after `dev` and `p` exist
    rgb8 = [b for b in blocks if "rt_render_rgb8" in b and "#include" not in b]
    assert rgb8, "the device-film snippet is gone from INTEGRATION.md"
    parts.append("inline void rgb8_variant(rt_scene *dev, rt_params p, Image &image) {\n" + rgb8[0] + "    (void)rc;\n}\n")
    parts.append("int main() { Scene s; Image img(4, 4, {1, 1, 1}); run_raytracer_amd(s, img); return 0; }\n")
    src.write_text("".join(parts))
    r = subprocess.run(["g++", "-std=c++20", "-fsyntax-only", "-I", REFERENCE_SRC, "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
