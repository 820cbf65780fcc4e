"""The preconditions of the light-group fixtures (tests/light_groups.py), asserted on the CPU oracle: the channel-separated scenes light most
pixels in every channel the exact check of tests/test_gpu_light_groups.py reads, the room's paths take every exit of shade() whose terminal
value or frame a tag owns, and changing emission colours changes no path (the twelve event counters stay what they were)."""
import numpy as np
import pytest

import light_groups as lg
from light_groups import COUNTERS, H, N, SEED, W


@pytest.fixture(scope="module")
def images(oracle, scenes):
    out = {}
    for name in ("room_plain", "boxes"):
        sc, _, _ = lg.channel_scene(scenes[name])
        orc = oracle.OracleScene(sc)
        fb, st = orc.run_raytracer(W, H, N, seed=SEED)
        out[name] = (fb, st, orc.shade_census_render(W, H, N, seed=SEED))
        orc.close()
    return out


def test_room_lights_most_pixels_in_both_light_channels(images):
    fb = images["room_plain"][0]
    share = [(fb[..., c] > 0).mean() for c in range(3)]
    print("room: share of pixels above zero per channel", share)
    assert share[0] >= 0.9 and share[1] >= 0.9


def test_boxes_mix_all_three_channels(images):
    fb = images["boxes"][0]
    share = [(fb[..., c] > 0).mean() for c in range(3)]
    every = (fb > 0).all(axis=2).mean()
    print("boxes: share of pixels above zero per channel", share, "all three", every)
    assert share[0] >= 0.2 and share[1] >= 0.2 and share[2] == 1.0 and every >= 0.1


def test_room_paths_take_every_exit_a_tag_owns(images):
    census = images["room_plain"][2]
    print({k: census[k] for k in lg.CENSUS_SLOTS})
    for slot in lg.CENSUS_SLOTS:
        assert census[slot] > 0, slot


@pytest.mark.parametrize("name", ["room_plain", "boxes"])
def test_paths_do_not_depend_on_emission_colours(oracle, scenes, images, name):
    orc = oracle.OracleScene(lg.plain_scene(scenes[name]))
    _, st = orc.run_raytracer(W, H, N, seed=SEED)
    orc.close()
    for key in COUNTERS:
        assert st[key] == images[name][1][key], key
    assert st["samples"] == W * H * N


def test_the_split_moves_every_second_light(scenes):
    sc, mg, bg = lg.channel_scene(scenes["room_plain"])
    base = scenes["room_plain"]
    lights = np.nonzero(base.material_ids == 1)[0]
    assert len(sc.materials) == len(base.materials) + 1 and bg == 2
    assert np.array_equal(np.nonzero(sc.material_ids == len(base.materials))[0], lights[::2])
    assert np.array_equal(np.nonzero(sc.material_ids == 1)[0], lights[1::2])
    assert sc.materials[1].emissive_strength == base.materials[1].emissive_strength == sc.materials[-1].emissive_strength
    assert [g for g in mg if g is not None] == [0, 1]
    assert base.materials[1].emission == (1.0, 0.95, 0.85) and base.bg_color == (1.0, 1.0, 1.0)  # the golden scene itself is untouched


def test_models_restate_the_rule():
    rng = np.random.default_rng(3)
    GS = rng.uniform(0, 4, size=(3, 2, 5, 3)).astype(np.float32)
    n = np.array([[0, 1, 2, 3, 8], [8, 8, 0, 5, 7]], dtype=np.uint32)
    w = rng.uniform(-1, 2, size=(3, 3)).astype(np.float32)
    got = lg.mix_model(GS, n, w)
    for y in range(2):
        for x in range(5):
            for c in range(3):
                acc = np.float32(0)
                for g in range(3):
                    m = np.float32(0) if n[y, x] == 0 else np.float32(GS[g, y, x, c] / np.float32(n[y, x]))
                    acc = np.float32(acc + np.float32(m * w[g, c]))
                assert got[y, x, c] == acc
    S = rng.uniform(0, 1, size=(2, 5, 3)).astype(np.float32)
    good = np.zeros((3, 2, 5, 3), np.float32)
    for k in range(3):
        good[k, ..., k] = S[..., k]
    good[1, 0, 0, 0] = -0.0  # a zero channel may hold -0
    lg.assert_channels(good, S)
    bad = good.copy()
    bad[2, 1, 1, 2] = np.nextafter(bad[2, 1, 1, 2], np.float32(9))
    with pytest.raises(AssertionError):
        lg.assert_channels(bad, S)
    bad = good.copy()
    bad[0, 1, 1, 1] = 1e-30
    with pytest.raises(AssertionError):
        lg.assert_channels(bad, S)
