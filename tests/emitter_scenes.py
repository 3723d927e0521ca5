"""The room of the emitter-sampling tests (rt_set_emitter_sampling), written through
scene_bin.write_bin so that every corner has its own vertex and the floor's smooth normal is (0, 1, 0):

  floor     8 x 8 quads at y = 0 over [-4, 4]^2           triangles [0, 128)     id 6  flat Lambertian, colour C
  lamp      2 x 2 quads at y = H_LAMP over [-0.5, 0.5]^2  triangles [128, 136)   id 0  EMISSIVE, emission E
  occluder  one quad at y = 1 over [1, 3] x [-1, 1]        triangles [136, 138)   id 7  flat Lambertian
  filler    one small quad at y = -50, seen by nothing     triangles [138, 140)   id 3

A floor point sees the whole lamp unless the occluder is in between, and then the lamp's shadow ray is
blocked for every point of the lamp or for some: both kinds of entry exist in one frame.  The filler
makes the count a multiple of 4.  The loader pads a mesh to one with index 0, as the reference does,
and with the 138 triangles of the three objects alone that has two effects the oracle shares and these
tests are not about: vertex 0's smooth normal takes in the two degenerate padding triangles and is NaN,
so the floor triangle that owns it shades to nothing; and rays do not reach the mesh's last two
triangles (oracle.intersect misses them too).
"""
import numpy as np

W, H = 96, 54
H_LAMP = 2.0
C = (0.5, 0.25, 0.75)
E = (1.0, 1.0, 1.0)
FLOOR, LAMP, OCCLUDER, FILLER = slice(0, 128), slice(128, 136), slice(136, 138), slice(138, 140)
N_TRIS = 140
ID_FLOOR, ID_LAMP, ID_OCCLUDER = 6, 0, 7
OCCLUDER_BOX = ((1.0, 3.0), (-1.0, 1.0))  # x and z ranges at y = 1
CAM_POS, CAM_YAW, CAM_PITCH = (0.0, 2.5, -5.5), 0.0, -0.5


def quads(x0, x1, z0, z1, y, nx, nz):
    """nx x nz quads of the rectangle at height y, two triangles each, geometric normal (0, 1, 0)."""
    xs = np.linspace(x0, x1, nx + 1, dtype=np.float32)
    zs = np.linspace(z0, z1, nz + 1, dtype=np.float32)
    tris = []
    for i in range(nx):
        for j in range(nz):
            a, b = (xs[i], y, zs[j]), (xs[i], y, zs[j + 1])
            c, d = (xs[i + 1], y, zs[j + 1]), (xs[i + 1], y, zs[j])
            tris.append([a, b, c])
            tris.append([a, c, d])
    return tris


def room_triangles(lamp_dx=0.0):
    """(140, 3, 3) float32; lamp_dx moves the lamp along x."""
    t = quads(-4.0, 4.0, -4.0, 4.0, 0.0, 8, 8)
    t += quads(-0.5 + lamp_dx, 0.5 + lamp_dx, -0.5, 0.5, H_LAMP, 2, 2)
    t += quads(OCCLUDER_BOX[0][0], OCCLUDER_BOX[0][1], OCCLUDER_BOX[1][0], OCCLUDER_BOX[1][1], 1.0, 1, 1)
    t += quads(-0.25, 0.25, -0.25, 0.25, -50.0, 1, 1)
    t = np.asarray(t, np.float32)
    assert t.shape == (N_TRIS, 3, 3)
    return t


def room_ids():
    ids = np.empty(N_TRIS, np.uint8)
    ids[FLOOR], ids[LAMP], ids[OCCLUDER], ids[FILLER] = ID_FLOOR, ID_LAMP, ID_OCCLUDER, 3
    return ids


def room_camera(rtx, oracle):
    """Looks along +z and down from in front of the room: the floor fills the lower two thirds of the
    frame, the lamp sits above the frustum's centre."""
    c = oracle.default_camera(W, H)
    c.pos[:] = CAM_POS
    c.yaw, c.pitch = CAM_YAW, CAM_PITCH
    r = None
    if rtx is not None:
        r = rtx.Camera()
        r.pos[:] = CAM_POS
        r.yaw, r.pitch, r.focal, r.aperture, r.fovX = CAM_YAW, CAM_PITCH, c.focal, c.aperture, c.fovX
    return c, r


def room_materials(rtx, emission=E):
    """{id: Material} of the three objects."""
    def make(base, **kw):
        m = rtx.default_material(base)
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(m, k)[:] = v
            else:
                setattr(m, k, v)
        return m

    return {ID_FLOOR: make(ID_FLOOR, type=rtx.MAT_LAMBERTIAN, flags=rtx.MAT_FLAG_FLAT, color=C),
            ID_OCCLUDER: make(ID_OCCLUDER, type=rtx.MAT_LAMBERTIAN, flags=rtx.MAT_FLAG_FLAT, color=(0.5, 0.5, 0.5)),
            ID_LAMP: make(ID_LAMP, type=rtx.MAT_EMISSIVE, emission=tuple(emission))}
