"""Helpers of the surface-query tests (rt_trace_surfaces_device): the ray set and the CPU oracle's
surface records for it, packed as the device packs them (include/rtx_amd.h).

The ray set is rays PICK u {N - 1} of test_gpu_ray_query.make_rays on the default scene: 4,097 rays,
not a multiple of 64 or 256.  On the CPU oracle: hit share 0.699, 1,948 front-face and 917 back-face
hits, 2,048 hits whose shading normal differs from the geometric one, 2,802 distinct triangles, 521
rays with a zeroed direction component.  ray_set asserts the bounds the tests rely on, so a changed
fixture cannot empty a case."""
import numpy as np

from test_gpu_ray_query import N, PICK, make_rays

SEL = np.concatenate([PICK, [N - 1]])
HIT_BIT, FRONT_BIT = 1 << 17, 1 << 16


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def oracle_hits(oracle, bvh, org, d):
    """(o, rec): oracle.intersect's hits, and their 16-B records (t, triangle, u, v of the closest hit
    itself: intersect_uv) as uint32 bit patterns."""
    o, uv = oracle.intersect_uv(bvh, np.concatenate([org, d], axis=1))
    rec = np.empty((len(org), 4), np.uint32)
    rec[:, 0] = bits(o["t"])
    rec[:, 1] = o["objectIdx"].view(np.uint32)
    rec[:, 2:4] = bits(uv)
    return o, rec


def pack_surfaces(o, material=3):
    """oracle.intersect's pos, offset, normal, ndr, fakeNormal, intoSurface and hit as the 12-float record,
    uint32 bit patterns.  material: one id, or an array of ids per triangle (ids[objectIdx])."""
    n = len(o)
    s = np.zeros((n, 12), np.uint32)
    s[:, 0:3] = bits(o["pos"])
    s[:, 3] = bits(o["offset"])
    s[:, 4:7] = bits(o["normal"])
    s[:, 7] = bits(o["ndr"])
    s[:, 8:11] = bits(o["fakeNormal"])
    hit = o["hit"] != 0
    mat = np.asarray(material)
    ids = np.full(n, int(mat), np.uint32) if mat.ndim == 0 else mat[np.maximum(o["objectIdx"], 0)].astype(np.uint32)
    word = (ids & 0xFFFF) | np.where(o["intoSurface"] != 0, FRONT_BIT, 0).astype(np.uint32) | np.uint32(HIT_BIT)
    s[:, 11] = np.where(hit, word, 0)
    return s


def oracle_surfaces(oracle, bvh, org, d, material=3):
    return pack_surfaces(oracle_hits(oracle, bvh, org, d)[0], material)


MISS = np.zeros(12, np.uint32)  # the surface of a miss
MISS[0:3] = bits(np.float32(10e10))[0]
MISS[3] = bits(np.float32(1e-7))[0]
MISS[4:7] = bits(np.array([0.0, -1.0, 0.0], np.float32))
MISS[7] = 0x80000000  # -0.0f
MISS[8:11] = MISS[4:7]

_cache = {}


def ray_set(oracle, scene):
    """The 4,097 rays with the oracle's hits, records and surfaces (material 3), computed once per scene."""
    key = id(scene)
    if key not in _cache:
        org, d = make_rays(scene["vertices"])
        org, d = np.ascontiguousarray(org[SEL]), np.ascontiguousarray(d[SEL])
        o, rec = oracle_hits(oracle, scene["bvh"], org, d)
        surf = pack_surfaces(o)
        hit = o["hit"] != 0
        front = hit & (o["intoSurface"] != 0)
        differs = hit & (o["normal"] != o["fakeNormal"]).any(1)
        assert len(org) == 4097 and 0.5 < hit.mean() < 0.95, hit.mean()
        assert front.sum() >= 500 and (hit & ~front).sum() >= 500, (front.sum(), (hit & ~front).sum())
        assert differs.sum() >= 1000, differs.sum()
        assert np.array_equal(surf[~hit], np.broadcast_to(MISS, ((~hit).sum(), 12)))
        r = dict(org=org, dir=d, o=o, rec=rec, surf=surf, hit=hit)
        for a in (org, d, o, rec, surf, hit):
            a.setflags(write=False)
        _cache[key] = (scene, r)  # the scene is kept, so its id is not reused
    return _cache[key][1]
