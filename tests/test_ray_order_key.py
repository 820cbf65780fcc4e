"""The ray-order key (csrc/rt_ray_key.h) as plain C++: a program compiled against the header checks, for every direction octant, every
ordering of |dx|, |dy|, |dz| (strict and tied) and the corner cells of the 64^3 grid, that

  * the key stays below RT_RAY_KEY_PAD = 0xFFFFFF: the ray-order sort runs over the queue's physical positions and the unfilled ends of the
    sub-queue regions hold pad entries BETWEEN real ones, so a pad must lose against every real key on the 24 compared bits alone;
  * the key is the formula wf_sort_keys used to carry (written out again in the program) with sub-cone 7 stored as 3, and the two sub-cone
    values that contradict transitivity, 3 and 4, never come out of finite components;
  * NaN components give a defined key: cell 0 on that axis, every comparison false, the same value on every call.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytracing-course-hw-public_amd", "csrc")

PROGRAM = r"""
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include "rt_ray_key.h"

static uint32_t spread3(uint32_t v) {
    v &= 63u;
    v = (v | (v << 8)) & 0x0300Fu;
    v = (v | (v << 4)) & 0x030C3u;
    v = (v | (v << 2)) & 0x09249u;
    return v;
}
// the formula as wf_sort_keys had it, sub-cone unrenumbered
static uint32_t old_key(const float *o, const float *d, const float *lo, const float *inv, uint32_t *sub_out) {
    const float fx = (o[0] - lo[0]) * inv[0], fy = (o[1] - lo[1]) * inv[1], fz = (o[2] - lo[2]) * inv[2];
    const uint32_t cx = (uint32_t)fminf(fmaxf(fx * 64.0f, 0.0f), 63.0f), cy = (uint32_t)fminf(fmaxf(fy * 64.0f, 0.0f), 63.0f), cz = (uint32_t)fminf(fmaxf(fz * 64.0f, 0.0f), 63.0f);
    const uint32_t morton = spread3(cx) | (spread3(cy) << 1) | (spread3(cz) << 2);
    const uint32_t oct = (d[0] < 0.0f ? 1u : 0u) | (d[1] < 0.0f ? 2u : 0u) | (d[2] < 0.0f ? 4u : 0u);
    const float ax = fabsf(d[0]), ay = fabsf(d[1]), az = fabsf(d[2]);
    const uint32_t sub = (ax > ay ? 1u : 0u) | (ay > az ? 2u : 0u) | (ax > az ? 4u : 0u);
    *sub_out = sub;
    return (oct << 21) | (morton << 3) | sub;
}

int main() {
    const float lo[3] = {-2.0f, 1.0f, 10.0f}, ext[3] = {4.0f, 0.5f, 100.0f};
    const float inv[3] = {1.0f / ext[0], 1.0f / ext[1], 1.0f / ext[2]};
    // origins: the two corner cells, beyond both corners (clamped), an inner cell
    const float fr[5] = {0.0f, 1.0f, -0.5f, 1.5f, 0.37f};
    // magnitudes: all 6 strict orderings and the ties come from choosing each component among three levels (27 triples), 0 included
    const float mag[4] = {0.0f, 0.25f, 0.5f, 1.0f};
    unsigned long n = 0, bad = 0, sevens = 0, corner_lo = 0, corner_hi = 0;
    bool seen_sub[8] = {false, false, false, false, false, false, false, false};
    for (int a = 0; a < 5; ++a)
        for (int b = 0; b < 5; ++b)
            for (int c = 0; c < 5; ++c) {
                const float o[3] = {lo[0] + fr[a] * ext[0], lo[1] + fr[b] * ext[1], lo[2] + fr[c] * ext[2]};
                for (int i = 0; i < 4; ++i)
                    for (int j = 0; j < 4; ++j)
                        for (int k = 0; k < 4; ++k)
                            for (int oct = 0; oct < 8; ++oct) {
                                const float d[3] = {(oct & 1) ? -mag[i] : mag[i], (oct & 2) ? -mag[j] : mag[j], (oct & 4) ? -mag[k] : mag[k]};
                                uint32_t sub;
                                const uint32_t was = old_key(o, d, lo, inv, &sub);
                                const uint32_t want = sub == 7u ? (was & ~7u) | 3u : was;
                                const uint32_t got = rt_ray_order_key(o[0], o[1], o[2], d[0], d[1], d[2], lo, inv);
                                ++n;
                                seen_sub[sub] = true;
                                sevens += sub == 7u;
                                if (got != want || got >= RT_RAY_KEY_PAD || (got >> RT_RAY_KEY_BITS) != 0u || sub == 3u || sub == 4u) {
                                    if (++bad <= 10)
                                        std::printf("BAD o %g %g %g d %g %g %g: got %06x want %06x sub %u\n", o[0], o[1], o[2], d[0], d[1], d[2], got, want, sub);
                                }
                                const uint32_t cell = (got >> 3) & 0x3FFFFu;
                                corner_lo += cell == 0u;
                                corner_hi += cell == 0x3FFFFu;
                            }
            }
    // the largest key there is: octant 7, cell (63, 63, 63), |dx| > |dy| > |dz|
    {
        const uint32_t top = rt_ray_order_key(lo[0] + ext[0], lo[1] + ext[1], lo[2] + ext[2], -1.0f, -0.5f, -0.25f, lo, inv);
        if (top != 0xFFFFFBu) {
            std::printf("BAD top key %06x\n", top);
            ++bad;
        }
    }
    // NaN: every component in turn and all at once, origin and direction; the key is defined (below the pad, equal on a second call) and is
    // what the rules give: cell 0 on a NaN axis, no octant bit and no comparison true for a NaN component
    const float nan = std::numeric_limits<float>::quiet_NaN();
    for (int m = 1; m < 64; ++m) {
        float v[6] = {lo[0] + 0.5f * ext[0], lo[1] + 0.5f * ext[1], lo[2] + 0.5f * ext[2], -1.0f, -0.5f, -0.25f};
        for (int q = 0; q < 6; ++q)
            if (m & (1 << q))
                v[q] = nan;
        const uint32_t k1 = rt_ray_order_key(v[0], v[1], v[2], v[3], v[4], v[5], lo, inv), k2 = rt_ray_order_key(v[0], v[1], v[2], v[3], v[4], v[5], lo, inv);
        const uint32_t cell = (k1 >> 3) & 0x3FFFFu, oct = k1 >> 21;
        bool ok = k1 == k2 && k1 < RT_RAY_KEY_PAD && (k1 & 7u) != 7u;
        for (int q = 0; q < 3; ++q) {
            if (m & (1 << q)) // cell coordinate q is 0: bits q, q + 3, ... of the Morton code are clear
                ok = ok && (cell & (0x9249u << q)) == 0u;
            if (m & (8 << q))
                ok = ok && (oct & (1u << q)) == 0u;
        }
        if ((m >> 3) == 7)
            ok = ok && (k1 & 7u) == 0u;
        ++n;
        if (!ok) {
            std::printf("BAD NaN mask %d: key %06x / %06x\n", m, k1, k2);
            ++bad;
        }
    }
    for (int s = 0; s < 8; ++s)
        if (seen_sub[s] != (s != 3 && s != 4)) {
            std::printf("BAD sub-cone %d %s\n", s, seen_sub[s] ? "seen" : "never seen");
            ++bad;
        }
    std::printf("checked %lu bad %lu sevens %lu corner_lo %lu corner_hi %lu\n", n, bad, sevens, corner_lo, corner_hi);
    return bad == 0 ? 0 : 1;
}
"""


def test_ray_order_key_as_plain_cpp(tmp_path):
    src, exe = tmp_path / "ray_key.cpp", tmp_path / "ray_key"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    last = r.stdout.strip().splitlines()[-1].split()
    stats = dict(zip(last[0::2], last[1::2]))  # "checked N bad 0 sevens S corner_lo A corner_hi B"
    assert int(stats["bad"]) == 0 and int(stats["checked"]) == 5 ** 3 * 4 ** 3 * 8 + 63
    assert int(stats["sevens"]) > 0 and int(stats["corner_lo"]) > 0 and int(stats["corner_hi"]) > 0  # the cases the renumbering and the pad are about
