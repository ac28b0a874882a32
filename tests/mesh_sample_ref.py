"""The rule of include/spann3r_hip.h "Mesh surface sampling and normals" in plain numpy: the anchor of every device comparison in
tests/test_mesh_sample_gpu.py, itself checked against a second formulation (a sample-by-sample loop over Python integers) and for
its statistics in tests/test_mesh_sample_cpu.py.  Open3D's sample_points_uniformly / compute_vertex_normals and trimesh's
sample_surface are not available: parity with them is unpinned.

The rule.  vertices fp32 [V, 3], rgba uint32 [V] (optional), faces int32 [F, 3].
1. Face frame.  A face is valid when its three indices lie in 0..V-1.  With its corners A, B, C in fp64: e1 = B - A, e2 = C - A,
   n = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x), d = sqrt(nx nx + ny ny + nz nz) summed left to right (twice the
   area), every operation rounded on its own.  An invalid face, or one whose d is not finite, has d = 0 and n = 0.  The unit face
   normal is fp32(n / d) per component, zeros when d = 0.  dmax = the largest d.
2. Weight.  w = uint64(floor(d / dmax * 2^32)) (0 when d = 0), at most 2^32; cum = the inclusive prefix sum of w in face order,
   uint64; W = its total.  A face with w = 0 -- invalid, degenerate or below 2^-32 of the largest -- is never drawn.  The quantised
   area is fp64(W) / 2^32 * dmax / 2.
3. h(c) = splitmix64 of seed + (c + 1) * 0x9E3779B97F4A7C15 modulo 2^64: z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9,
   z = (z ^ z >> 27) * 0x94D049BB133111EB, z ^ z >> 31.
4. Sample k: t = (h(3k) * W) >> 64, face = the smallest f with cum[f] > t; a = h(3k + 1) >> 40, b = h(3k + 2) >> 40 and, if
   a + b > 2^24, a = 2^24 - a, b = 2^24 - b; point per axis = fp32(fp64(A) + (a / 2^24 * e1 + b / 2^24 * e2)), the two products,
   the two sums and the narrowing each rounded on their own; colour per byte (cA (2^24 - a - b) + cB a + cC b + 2^23) >> 24; the
   sample's normal is its face's unit normal.
5. Vertex normals.  Per valid face and component q = rint(n_c / dmax * 2^30) (half to even), added to each of the face's three
   vertices in int64; normal = fp32(S_c / sqrt(Sx Sx + Sy Sy + Sz Sz)) with S in fp64, zeros when all three sums are 0."""
import numpy as np

GOLDEN = 0x9E3779B97F4A7C15
M1, M2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
TWO32, TWO30, TWO24 = 4294967296.0, 1073741824.0, 1 << 24


def _corners(vertices, faces):
    """-> (valid bool [F], A, e1, e2 fp64 [F, 3]); the rows of invalid faces come from vertex 0 and are masked by the callers"""
    v = np.asarray(vertices, np.float32).reshape(-1, 3).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    valid = ((f >= 0) & (f < len(v))).all(1)
    if len(v) == 0:
        z = np.zeros((len(f), 3), np.float64)
        return valid, z, z.copy(), z.copy()
    g = np.where(valid[:, None], f, 0)
    a, b, c = v[g[:, 0]], v[g[:, 1]], v[g[:, 2]]
    with np.errstate(all="ignore"):
        return valid, a, b - a, c - a


def face_frames(vertices, faces):
    """-> dict(n fp64 [F, 3], d fp64 [F], face_normals fp32 [F, 3], dmax fp64, w uint64 [F], cum uint64 [F], W int, area float)"""
    valid, _, e1, e2 = _corners(vertices, faces)
    with np.errstate(all="ignore"):
        n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
        d = np.sqrt(n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2])
        ok = valid & np.isfinite(d)
        d = np.where(ok, d, 0.0)
        n = np.where(ok[:, None], n, 0.0)
        pos = d > 0
        unit = np.where(pos[:, None], n / np.where(pos, d, 1.0)[:, None], 0.0).astype(np.float32)
        dmax = np.float64(d.max()) if len(d) else np.float64(0.0)
        w = np.where(pos, np.floor(d / (dmax if dmax > 0 else 1.0) * TWO32), 0.0).astype(np.uint64)
    cum = np.cumsum(w, dtype=np.uint64)
    W = int(cum[-1]) if len(cum) else 0
    return dict(n=n, d=d, face_normals=unit, dmax=dmax, w=w, cum=cum, W=W, area=float(np.float64(W) / TWO32 * dmax / 2.0))


def h(counters, seed=0):
    """the counter-based generator: uint64 array of counters -> uint64 array"""
    c = np.asarray(counters, np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(int(seed) & (2 ** 64 - 1)) + (c + np.uint64(1)) * np.uint64(GOLDEN)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(M1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(M2)
    return z ^ (z >> np.uint64(31))


def umulhi64(x, y):
    """the high 64 bits of the 128-bit products x * y, from 32-bit halves"""
    x, y = np.asarray(x, np.uint64), np.asarray(y, np.uint64)
    lo32, s32 = np.uint64(0xFFFFFFFF), np.uint64(32)
    x0, x1, y0, y1 = x & lo32, x >> s32, y & lo32, y >> s32
    mid = x1 * y0 + ((x0 * y0) >> s32)                       # < 2^64: (2^32 - 1)^2 + 2^32 - 1
    mid2 = x0 * y1 + (mid & lo32)
    return x1 * y1 + (mid >> s32) + (mid2 >> s32)


def sample(vertices, rgba, faces, n, seed=0, frames=None):
    """-> dict(points fp32 [n, 3], normals fp32 [n, 3], rgba uint32 [n] or None, face_index int32 [n]); W = 0 with n > 0 raises"""
    fr = face_frames(vertices, faces) if frames is None else frames
    n = int(n)
    if n > 0 and fr["W"] == 0:
        raise ValueError("mesh_sample_ref.sample: the mesh has no area to sample")
    k = np.arange(n, dtype=np.uint64) * np.uint64(3)
    if n == 0:
        return dict(points=np.zeros((0, 3), np.float32), normals=np.zeros((0, 3), np.float32), face_index=np.zeros(0, np.int32),
                    rgba=None if rgba is None else np.zeros(0, np.uint32))
    t = umulhi64(h(k, seed), np.uint64(fr["W"]))
    face = np.searchsorted(fr["cum"], t, side="right").astype(np.int64)
    a = (h(k + np.uint64(1), seed) >> np.uint64(40)).astype(np.int64)
    b = (h(k + np.uint64(2), seed) >> np.uint64(40)).astype(np.int64)
    flip = a + b > TWO24
    a, b = np.where(flip, TWO24 - a, a), np.where(flip, TWO24 - b, b)
    _, A, e1, e2 = _corners(vertices, faces)
    ua, ub = (a.astype(np.float64) / np.float64(TWO24))[:, None], (b.astype(np.float64) / np.float64(TWO24))[:, None]
    points = (A[face] + (ua * e1[face] + ub * e2[face])).astype(np.float32)
    col = None
    if rgba is not None:
        c = np.asarray(rgba).astype(np.uint32).reshape(-1)[np.asarray(faces, np.int64).reshape(-1, 3)[face]].astype(np.int64)      # [n, 3]
        col = np.zeros(n, np.int64)
        for byte in range(4):
            ca, cb, cc = ((c[:, j] >> (8 * byte)) & 255 for j in range(3))
            col |= ((ca * (TWO24 - a - b) + cb * a + cc * b + (1 << 23)) >> 24) << (8 * byte)
        col = col.astype(np.uint32)
    return dict(points=points, normals=fr["face_normals"][face], rgba=col, face_index=face.astype(np.int32))


def vertex_sums(vertices, faces, frames=None):
    """-> int64 [V, 3]: the integer sums of step 5"""
    fr = face_frames(vertices, faces) if frames is None else frames
    nv = len(np.asarray(vertices).reshape(-1, 3))
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    sums = np.zeros((nv, 3), np.int64)
    use = fr["d"] > 0
    if use.any():
        q = np.rint(fr["n"][use] / fr["dmax"] * TWO30).astype(np.int64)
        for j in range(3):
            np.add.at(sums, f[use, j], q)
    return sums


def vertex_normals(vertices, faces, frames=None):
    """-> fp32 [V, 3]"""
    s = vertex_sums(vertices, faces, frames).astype(np.float64)
    length = np.sqrt(s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1] + s[:, 2] * s[:, 2])
    zero = (s == 0).all(1)
    return np.where(zero[:, None], 0.0, s / np.where(zero, 1.0, length)[:, None]).astype(np.float32)
