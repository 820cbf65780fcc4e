"""CPU tests of the float environment: the float decode of Radiance HDR pictures (rt_hdr_decode_file_float / rt.load_hdr) against an RGBE
decode written here, and the numpy restatement of the distribution (tests/env_replay.py) against the properties the rule promises."""
import os
import re

import numpy as np
import pytest

import env_replay as er

HERE = os.path.dirname(os.path.abspath(__file__))
ENV = os.path.join(HERE, "golden", "envmap")
SEED = 20261019


def rgbe_decode(path):
    """Radiance RGBE, from the file format: header lines up to the empty one, '-Y h +X w', then flat quadruples or, for 8 <= w < 32768 and a
    scanline starting 2 2 hi lo, the four components run-length coded one after the other. value = mantissa * 2^(e - 136), 0 for e = 0."""
    data = open(path, "rb").read()
    head, _, rest = data.partition(b"\n\n")
    assert head.startswith(b"#?RADIANCE") or head.startswith(b"#?RGBE")
    dims, _, px = rest.partition(b"\n")
    m = re.match(rb"-Y (\d+) \+X (\d+)", dims)
    h, w = int(m.group(1)), int(m.group(2))
    quads = np.zeros((h, w, 4), dtype=np.uint8)
    pos = 0
    rle = 8 <= w < 32768 and px[0] == 2 and px[1] == 2 and not (px[2] & 0x80)
    if not rle:
        quads = np.frombuffer(px[:h * w * 4], dtype=np.uint8).reshape(h, w, 4).copy()
    else:
        for y in range(h):
            assert px[pos] == 2 and px[pos + 1] == 2 and (px[pos + 2] << 8 | px[pos + 3]) == w
            pos += 4
            for k in range(4):
                x = 0
                while x < w:
                    count = px[pos]
                    pos += 1
                    if count > 128:
                        quads[y, x:x + count - 128, k] = px[pos]
                        pos += 1
                        x += count - 128
                    else:
                        quads[y, x:x + count, k] = np.frombuffer(px[pos:pos + count], dtype=np.uint8)
                        pos += count
                        x += count
    e = quads[..., 3].astype(np.int32)
    scale = np.where(e != 0, np.ldexp(1.0, e - 136), 0.0)  # float64: exact
    return (quads[..., :3].astype(np.float64) * scale[..., None]).astype(np.float32)  # 8-bit mantissa x power of two: exact in float32


@pytest.mark.parametrize("name", ["env_flat", "env_narrow", "env_rle", "env_wide"])
def test_float_hdr_decode_is_the_rgbe_value_bit_for_bit(rt, name):
    """(a) rt.load_hdr returns mantissa * 2^(e - 136) exactly, zeros for e = 0, with nothing clipped: the fixtures' sun is above 1."""
    path = os.path.join(ENV, name + ".hdr")
    got = rt.load_hdr(path)
    want = rgbe_decode(path)
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert got.max() > 1.0  # what the 8-bit load (to_ldr) clips away
    ldr = rt.image_decode(path)  # the parity path is untouched: still the 8-bit conversion
    assert ldr.dtype == np.uint8 and ldr.shape[:2] == got.shape[:2]


def test_load_hdr_of_an_8_bit_picture_applies_the_lookup_gamma(rt):
    png = os.path.join(ENV, "env.png")
    got = rt.load_hdr(png)
    texels = rt.image_decode(png)
    want = np.power((np.arange(256, dtype=np.float32) / np.float32(255.0)).astype(np.float64), 2.2)[texels[..., :3]]
    assert got.shape == want.shape and np.allclose(got, want, rtol=1e-6, atol=0)  # powf against float64 pow: a float rounding apart


def maps():
    rng = np.random.default_rng(SEED)
    isolated = np.zeros((8, 16, 3), dtype=np.float32)  # bright texels beside exact zeros
    for (y, x) in [(2, 3), (5, 9), (6, 15), (3, 0)]:
        isolated[y, x] = (50.0, 40.0, 30.0)
    pole = np.zeros((8, 16, 3), dtype=np.float32)  # a bright texel in each pole row
    pole[0, 4] = (20.0, 20.0, 20.0)
    pole[7, 11] = (0.0, 30.0, 0.0)
    seam = np.zeros((8, 16, 3), dtype=np.float32)  # bright texels on both sides of the u seam
    seam[3, 15] = (10.0, 0.0, 0.0)
    seam[4, 0] = (0.0, 0.0, 90.0)
    noise = (rng.random((16, 32, 3)) ** 6 * 30.0).astype(np.float32)
    return {"isolated": isolated, "pole": pole, "seam": seam, "noise": noise, "sky": er.sky()}


@pytest.mark.parametrize("name", ["isolated", "pole", "seam", "noise", "sky"])
def test_cell_probabilities_sum_to_one(name):
    """(b) the p_ij defined from the stored float tables sum to 1 to 1e-6."""
    t = er.Tables(maps()[name], bg=(1.0, 0.8, 1.2))
    assert t.ok
    assert abs(float(t.p.astype(np.float64).sum()) - 1.0) <= 1e-6
    assert (np.diff(t.marg) >= 0).all() and (np.diff(t.rows, axis=1) >= 0).all()
    assert t.marg[0] == 0 and t.marg[-1] == 1 and (t.rows[:, 0] == 0).all() and (t.rows[:, -1] == 1).all()


@pytest.mark.parametrize("name", ["isolated", "pole", "seam"])
def test_pdf_is_positive_wherever_the_radiance_is(name):
    """(c) 1e5 random directions: wherever the float64 bilinear radiance is > 0 the cell's pdf is > 0, because the weight takes the largest
    luminance over every texel a lookup in the cell reads."""
    tex = maps()[name]
    t = er.Tables(tex)
    d = np.random.default_rng(SEED + 1).normal(size=(100000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    le, ok, _ = er.radiance64(tex, (1.0, 1.0, 1.0), d)
    i, j, _ = er.cell_of(d, t.W, t.H)
    lit = ok & (le.sum(axis=1) > 0)
    assert lit.sum() > 1000 and (~lit).sum() > 1000  # both kinds of direction are really there
    assert (t.pdf_cells[i[lit], j[lit]] > 0).all()


def test_prefix_order_is_the_chunked_one():
    """The rule's prefix sums, spelled out with Python floats for one awkward length, equal the vectorised restatement bit for bit."""
    a = np.random.default_rng(SEED + 2).random(1000) ** 8
    C = -(-1000 // 256)
    want, base = [], 0.0
    for c in range(256):
        acc = 0.0
        for k in range(c * C, min(1000, (c + 1) * C)):
            acc += float(a[k])
            want.append(base + acc)
        base += acc
    P, total = er.prefix(a)
    assert np.array_equal(P, np.array(want)) and total == base


def test_replay_sampler_histogram_matches_the_cell_probabilities():
    """(d) 1e6 samples of the replay on a 32 x 16 map: every cell's frequency within 6 sqrt(p (1 - p) / N) + 1 / N of p_ij, and every sample
    lies in the cell it was drawn for when its direction goes back through (u, v)."""
    t = er.Tables(er.sky())
    n = 1000000
    xi = np.random.default_rng(SEED + 3).random((n, 4), dtype=np.float32)
    d, i, j = er.sample(t, xi)
    ok, worst = er.histogram_ok(i, j, t.p, n)
    assert ok, worst
    bi, bj, edge = er.cell_of(d, t.W, t.H)
    inside = edge > 1e-4
    assert inside.mean() > 0.99
    assert np.array_equal(bi[inside], i[inside]) and np.array_equal(bj[inside], j[inside])
    assert (t.pdf_cells[i, j] > 0).all()


def test_all_zero_map_has_no_distribution():
    t = er.Tables(np.zeros((4, 8, 3), dtype=np.float32))
    assert not t.ok
