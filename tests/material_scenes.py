"""Scenes, tables and expectations of the per-triangle material tests (rt_set_triangle_materials).

The oracle knows one scene-wide material (materialOverride), so a mixed frame gets its exact
expectation by construction ("Per-triangle materials"):

  * a table of one id equals that override;
  * ids of one type render alike but for the mask, so a table mixing them equals the override frame
    of the type with the mask taken from the table at sample 0's triangle;
  * on the cube below no path that starts on a face touches another face (the faces of a convex
    body do not see each other, and neither the mirror nor the diffuse bounces go inwards), so a
    table with one id per face gives, at every pixel, the override frame of that pixel's face.
    test_materials_api.py checks that premise on the oracle itself.
"""
import numpy as np

CUBE_W, CUBE_H = 96, 54
CUBE_FACES = ("x-", "x+", "y-", "y+", "z-", "z+")
CUBE_QUADS = 8
CUBE_FACE_TRIS = 2 * CUBE_QUADS * CUBE_QUADS   # 128
CUBE_VISIBLE = {"x+": 537, "y+": 387, "z-": 529}  # pixels of the cube camera per face
SKY_MASK = 99999 & 0xFFFF


def cube_triangles():
    """[-1, 1]^3 as 6 faces (x-, x+, y-, y+, z-, z+) of 8 x 8 quads, two triangles (0,1,2), (0,2,3)
    per quad over the corners (a,b), (a+1,b), (a+1,b+1), (a,b+1) in the face's two free axes:
    768 triangles, face f holding triangles [128 f, 128 f + 128)."""
    step = np.float32(2.0 / CUBE_QUADS)
    tris = []
    for axis in range(3):
        free = [k for k in range(3) if k != axis]
        for sign in (-1.0, 1.0):
            for a in range(CUBE_QUADS):
                for b in range(CUBE_QUADS):
                    corners = []
                    for da, db in ((0, 0), (1, 0), (1, 1), (0, 1)):
                        p = np.zeros(3, np.float32)
                        p[axis] = sign
                        p[free[0]] = np.float32(-1.0) + step * np.float32(a + da)
                        p[free[1]] = np.float32(-1.0) + step * np.float32(b + db)
                        corners.append(p)
                    tris.append([corners[0], corners[1], corners[2]])
                    tris.append([corners[0], corners[2], corners[3]])
    return np.asarray(tris, np.float32)


def cube_camera(rtx, oracle, k=0):
    """The cube camera (frame k of a slowly moving sequence; k = 0 is the one the pixel counts are of)."""
    pos = (2.2 + 0.02 * k, 1.9 + 0.01 * k, -2.2)
    yaw, pitch = 5.495 + 0.004 * k, -0.55
    c = oracle.default_camera(CUBE_W, CUBE_H)
    c.pos[:] = pos
    c.yaw, c.pitch = yaw, pitch
    r = None
    if rtx is not None:
        r = rtx.Camera()
        r.pos[:] = pos
        r.yaw, r.pitch, r.focal, r.aperture, r.fovX = yaw, pitch, c.focal, c.aperture, c.fovX
    return c, r


def face_table(assign, default=3):
    """uint8[768]: id assign[face] on the named faces, `default` elsewhere."""
    t = np.full(len(CUBE_FACES) * CUBE_FACE_TRIS, default, np.uint8)
    for face, mid in assign.items():
        f = CUBE_FACES.index(face)
        t[f * CUBE_FACE_TRIS:(f + 1) * CUBE_FACE_TRIS] = mid
    return t


def primary_triangles(oracle, bvh, w, h, cam, frame=1):
    """Sample 0's hit triangle per pixel (-1: sky) of frame `frame` at spp 1."""
    rays, _ = oracle.primary_rays(w, h, frame, cam)
    return oracle.intersect(bvh, rays)["objectIdx"].astype(np.int64)


def hashed_ids(n, palette):
    """palette[(k * 2654435761 >> 7) % len(palette)] for triangle k: ids scattered over the mesh."""
    k = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761)) >> np.uint64(7)
    return np.asarray(palette, np.uint8)[(k % np.uint64(len(palette))).astype(np.int64)]


def compose_by_pixel(frames, pick):
    """G-buffers whose pixel p is frames[pick[p]]'s."""
    keys = sorted(set(pick.tolist()))
    out = {}
    for name in frames[keys[0]]:
        a = frames[keys[0]][name].copy()
        for k in keys[1:]:
            sel = pick == k
            a[sel] = frames[k][name][sel]
        out[name] = a
    return out
