"""A host model of the id tables of an accumulator with ids (include/rt_abi.h, rt_accum_attach_ids), for exact comparisons with the device.
A plain module next to the tests (imported like feature_replay.py); everything is integer arithmetic except the two final divisions.
  sample_ids   the id of every sample from the closest hits of its primary ray (feature_replay.primary_rays + first_hits: the oracle's cast_rays);
  tables       the K first-seen slots and the overflow counter of every pixel after every prefix of its samples: level m = the first m samples;
  labels       rt_accum_resolve_labels of a table;
  matte        rt_accum_resolve_matte of a table."""
import numpy as np

MISS = 0xFFFFFFFF  # RT_ID_MISS, and what cast_rays reports for a ray that hits nothing


def sample_ids(prim, kind="primitive", material_ids=None, prim_materials=(), table=None):
    """prim (P, n) uint32 as cast_rays reports it (MISS, an original triangle index, or n_triangles + i for analytic primitive i) -> ids (P, n).
    kind "primitive": prim itself; "material": material_ids of the triangle, prim_materials[i] of the analytic primitive; "user": table[prim]."""
    prim = np.asarray(prim, dtype=np.uint32)
    hit = prim != MISS
    k = np.where(hit, prim, 0).astype(np.int64)
    if kind == "primitive":
        lut = None
    elif kind == "material":
        lut = np.concatenate([np.asarray(material_ids, dtype=np.uint32).reshape(-1), np.asarray(prim_materials, dtype=np.uint32).reshape(-1)])
    elif kind == "user":
        lut = np.asarray(table, dtype=np.uint32).reshape(-1)
    else:
        raise ValueError(kind)
    ids = prim if lut is None else lut[k]
    return np.where(hit, ids, np.uint32(MISS)).astype(np.uint32)


def tables(ids, K):
    """ids (P, n) uint32, K slots -> (slot ids (n + 1, P, K), counts (n + 1, P, K), other (n + 1, P)), all uint32: the rule of rt_abi.h, one
    sample at a time in sample order; level m holds the table of samples 0 .. m - 1."""
    ids = np.asarray(ids, dtype=np.uint32)
    P, n = ids.shape
    sid, cnt, other = np.zeros((P, K), np.uint32), np.zeros((P, K), np.uint32), np.zeros(P, np.uint32)
    L_id, L_cnt, L_other = [sid.copy()], [cnt.copy()], [other.copy()]
    r = np.arange(P)
    for s in range(n):
        x = ids[:, s]
        match = (cnt > 0) & (sid == x[:, None])
        found, jm = match.any(axis=1), match.argmax(axis=1)
        empty = cnt == 0
        room, je = empty.any(axis=1), empty.argmax(axis=1)  # argmax: the lowest such j
        cnt[r[found], jm[found]] += 1
        take = ~found & room
        sid[r[take], je[take]] = x[take]
        cnt[r[take], je[take]] = 1
        other[~found & ~room] += 1
        L_id.append(sid.copy()), L_cnt.append(cnt.copy()), L_other.append(other.copy())
    return np.stack(L_id), np.stack(L_cnt), np.stack(L_other)


def at(lad, n):
    """Level n_p of a ladder (L + 1, P, ...) for every pixel: n (H, W) -> (H, W, ...)."""
    n = np.asarray(n).astype(np.int64)
    flat = lad[n.reshape(-1), np.arange(n.size)]
    return flat.reshape(n.shape + lad.shape[2:])


def labels(sid, cnt, n):
    """sid, cnt (..., K), n (...) -> (label (...) uint32, coverage (...) float32): the fullest slot, ties to the lowest; MISS and 0 where n = 0."""
    sid, cnt, n = np.asarray(sid, np.uint32), np.asarray(cnt, np.uint32), np.asarray(n, np.uint32)
    j = cnt.argmax(axis=-1)[..., None]  # the first maximum
    lab, c = np.take_along_axis(sid, j, axis=-1)[..., 0], np.take_along_axis(cnt, j, axis=-1)[..., 0]
    with np.errstate(all="ignore"):
        cov = c.astype(np.float32) / n.astype(np.float32)
    return np.where(n > 0, lab, np.uint32(MISS)).astype(np.uint32), np.where(n > 0, cov, np.float32(0)).astype(np.float32)


def matte(sid, cnt, n, id_set):
    """The counts of the slots whose id is in id_set, summed as integers, over n; 0 where n = 0. A slot with count 0 holds nothing."""
    sid, cnt, n = np.asarray(sid, np.uint32), np.asarray(cnt, np.uint32), np.asarray(n, np.uint32)
    inside = np.isin(sid, np.asarray(id_set, dtype=np.uint32)) & (cnt > 0)
    total = np.where(inside, cnt, 0).sum(axis=-1, dtype=np.uint32)
    with np.errstate(all="ignore"):
        m = total.astype(np.float32) / n.astype(np.float32)
    return np.where(n > 0, m, np.float32(0)).astype(np.float32)


def distinct_per_pixel(ids):
    """ids (P, n) -> (P,) the number of distinct ids among each pixel's samples."""
    s = np.sort(np.asarray(ids, dtype=np.uint32), axis=1)
    return 1 + (s[:, 1:] != s[:, :-1]).sum(axis=1)


def user_table(n):
    """The user table of the tests: prim % 5, every 7th entry RT_ID_MISS."""
    t = (np.arange(n) % 5).astype(np.uint32)
    t[::7] = MISS
    return t
