"""The host model of the id tables (tests/id_replay.py) against the rule of include/rt_abi.h (rt_accum_attach_ids), and the preconditions of
the GPU cases of test_gpu_ids.py, asserted from the oracle: a fixture that stops exercising a branch fails here, without a GPU."""
import numpy as np
import pytest

import feature_replay as fr
import id_replay as ir

W, H, N = 64, 48, 8
SEED = 7


def _random_ids(P=200, n=12, distinct=5, seed=3):
    rng = np.random.default_rng(seed)
    pool = np.array([0, 7, ir.MISS, 3, 1 << 31, 12, 99], np.uint32)[:distinct]
    return pool[rng.integers(0, distinct, size=(P, n))]


# ------------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize("K", [1, 2, 4, 8, 16])
def test_counts_and_other_add_up_at_every_level(K):
    ids = _random_ids()
    sid, cnt, other = ir.tables(ids, K)
    assert sid.shape == cnt.shape == (13, 200, K) and other.shape == (13, 200)
    for m in range(13):
        assert np.all(cnt[m].sum(axis=1) + other[m] == m)
    assert np.all(sid[cnt == 0] == 0)  # an empty slot reads id 0
    assert (other[12] > 0).any() == (K < 5)


def test_enough_slots_give_the_histogram():
    ids = _random_ids(distinct=5)
    sid, cnt, other = ir.tables(ids, 8)
    assert not other.any()
    for p in range(ids.shape[0]):
        vals, first, hist = np.unique(ids[p], return_index=True, return_counts=True)
        order = np.argsort(first)  # first-seen order
        k = len(vals)
        assert np.array_equal(sid[-1, p, :k], vals[order]) and np.array_equal(cnt[-1, p, :k], hist[order])
        assert not cnt[-1, p, k:].any() and not sid[-1, p, k:].any()


@pytest.mark.parametrize("K", [1, 3, 16])
def test_a_level_is_the_table_of_that_prefix(K):
    ids = _random_ids()
    full = ir.tables(ids, K)
    for m in (0, 1, 5, 12):
        part = ir.tables(ids[:, :m], K)
        for a, b in zip(full, part):
            assert np.array_equal(a[m], b[m])


def test_one_slot_keeps_the_first_id():
    ids = _random_ids()
    sid, cnt, other = ir.tables(ids, 1)
    assert np.array_equal(sid[-1, :, 0], ids[:, 0])
    assert np.array_equal(cnt[-1, :, 0], (ids == ids[:, :1]).sum(axis=1))
    assert np.array_equal(other[-1], (ids != ids[:, :1]).sum(axis=1))


def test_id_zero_and_miss_are_ids_like_any_other():
    ids = np.array([[0, 0, ir.MISS, 0, ir.MISS, 5]], np.uint32)
    sid, cnt, other = ir.tables(ids, 2)
    assert sid[-1].tolist() == [[0, ir.MISS]] and cnt[-1].tolist() == [[3, 2]] and other[-1].tolist() == [1]
    assert sid[1].tolist() == [[0, 0]] and cnt[1].tolist() == [[1, 0]]  # id 0 in a taken slot, id 0 of an empty one


def test_labels_ties_go_to_the_lowest_slot_and_other_is_not_consulted():
    sid = np.array([[9, 4, 2, 0], [9, 4, 2, 0], [0, 0, 0, 0], [3, 8, 0, 0]], np.uint32)
    cnt = np.array([[2, 3, 3, 0], [1, 1, 1, 0], [0, 0, 0, 0], [1, 1, 0, 0]], np.uint32)
    n = np.array([8, 3, 0, 9], np.uint32)  # the last pixel: other = 7, and still the label is slot 0's
    lab, cov = ir.labels(sid, cnt, n)
    assert lab.tolist() == [4, 9, ir.MISS, 3]
    assert fr.same_bits(cov, np.array([3, 1, 0, 1], np.float32) / np.array([8, 3, 1, 9], np.float32))
    assert cov[2] == 0


def test_matte_sums_integers_and_ignores_duplicates_and_empty_slots():
    sid = np.array([[9, 4, ir.MISS, 0], [0, 0, 0, 0], [0, 5, 0, 0]], np.uint32)
    cnt = np.array([[2, 3, 1, 0], [0, 0, 0, 0], [1, 2, 0, 0]], np.uint32)
    n = np.array([7, 0, 3], np.uint32)
    m = ir.matte(sid, cnt, n, [4, ir.MISS, 4, 77])
    assert fr.same_bits(m, np.array([np.float32(4) / np.float32(7), 0, 0], np.float32))
    m0 = ir.matte(sid, cnt, n, [0])  # id 0: the taken slot of pixel 2 counts, the empty slots (id 0, count 0) of pixels 0 and 1 do not
    assert fr.same_bits(m0, np.array([0, 0, np.float32(1) / np.float32(3)], np.float32))


def test_sample_ids_kinds():
    prim = np.array([[0, 2, ir.MISS, 4, 3]], np.uint32)  # 3 triangles + 2 analytic primitives
    assert ir.sample_ids(prim).tolist() == [[0, 2, ir.MISS, 4, 3]]
    assert ir.sample_ids(prim, "material", material_ids=[5, 6, 7], prim_materials=[1, 9]).tolist() == [[5, 7, ir.MISS, 9, 1]]
    assert ir.sample_ids(prim, "user", table=[10, 11, ir.MISS, 13, 14]).tolist() == [[10, ir.MISS, ir.MISS, 14, 13]]


# ------------------------------------------------------------------------------------------------ the preconditions of the GPU cases
@pytest.fixture(scope="module")
def prims(oracle, scenes):
    cache = {}

    def get(name):
        if name not in cache:
            orc = oracle.OracleScene(scenes[name])
            _, _, prim = fr.first_hits(orc, fr.primary_rays(orc, W, H, N, SEED))
            orc.close()
            cache[name] = prim
        return cache[name]

    return get


def test_room_plain_overflows_small_tables_and_fits_eight_slots(prims, scenes):
    ids = ir.sample_ids(prims("room_plain"))
    d = ir.distinct_per_pixel(ids)
    print("room_plain primitive: distinct ids per pixel:", dict(zip(*[a.tolist() for a in np.unique(d, return_counts=True)])))
    for K in (1, 2, 4):  # other > 0 somewhere: the overflow branch
        assert (d > K).any(), K
    assert d.max() <= 8  # K = 8 and 16: other == 0 everywhere
    for K in (1, 2, 4, 8, 16):
        _, _, other = ir.tables(ids, K)
        assert other[N].any() == (K < 8)
    # a pixel whose first two samples differ: the label of level 2 is a tie, decided by the slot order
    assert (ids[:, 0] != ids[:, 1]).any()
    # material ids merge triangles: fewer distinct ids, and still more than one somewhere
    dm = ir.distinct_per_pixel(ir.sample_ids(prims("room_plain"), "material", material_ids=scenes["room_plain"].material_ids))
    assert 1 < dm.max() <= d.max()


def test_open_scene_has_pixels_that_see_a_hit_and_a_miss(prims):
    ids = ir.sample_ids(prims("open_nolight"))
    miss = ids == ir.MISS
    both = miss.any(axis=1) & (~miss).any(axis=1)
    print(f"open_nolight: {miss.mean():.3f} misses; {int(both.sum())} pixels see a hit and a miss; max distinct {int(ir.distinct_per_pixel(ids).max())}")
    assert both.any() and miss.all(axis=1).any()
    sid, cnt, other = ir.tables(ids, 2)
    held = ((sid[N] == ir.MISS) & (cnt[N] > 0)).any(axis=1) & ((sid[N] != ir.MISS) & (cnt[N] > 0)).any(axis=1)
    assert held.any()  # RT_ID_MISS beside a real id in one table
    assert other[N].any()  # and a pixel with three ids: the K = 2 table overflows


def test_room_textured_material_and_user_ids(prims, scenes):
    sc = scenes["room_textured"]
    prim = prims("room_textured")
    mat = ir.sample_ids(prim, "material", material_ids=sc.material_ids)
    assert ir.distinct_per_pixel(mat).max() >= 2 and len(np.unique(mat)) >= 3
    tab = ir.user_table(len(sc.material_ids))
    usr = ir.sample_ids(prim, "user", table=tab)
    assert (prim != ir.MISS).all()  # a closed room: every RT_ID_MISS below comes from the table
    miss = usr == ir.MISS
    assert miss.any() and (miss.any(axis=1) & (~miss).any(axis=1)).any()
    assert ir.distinct_per_pixel(usr).max() >= 3
    assert set(np.unique(usr).tolist()) <= {0, 1, 2, 3, 4, ir.MISS}


def test_scene000_analytic_primitives_win_primary_rays(rt, oracle):
    from conftest import SCENE000

    ls = rt.parse_scene_txt(SCENE000)
    a = ls.arrays()
    assert len(a["material_ids"]) == 12 and [p["kind"] for p in a["primitives"]] == [rt._ctypes_abi.RT_PRIM_ELLIPSOID, rt._ctypes_abi.RT_PRIM_PLANE]
    orc = oracle.OracleScene(ls)
    _, _, prim = fr.first_hits(orc, fr.primary_rays(orc, W, H, N, SEED))
    orc.close()
    assert (prim == 12).any() and (prim == 13).any()
    mat = ir.sample_ids(prim, "material", material_ids=a["material_ids"], prim_materials=[p["material_id"] for p in a["primitives"]])
    assert (mat[prim == 12] == a["primitives"][0]["material_id"]).all() and (mat[prim == 13] == a["primitives"][1]["material_id"]).all()
