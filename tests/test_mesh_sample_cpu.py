"""tests/mesh_sample_ref.py, the numpy restatement of include/spann3r_hip.h "Mesh surface sampling and normals", checked on its own:
against a sample-by-sample loop over Python integers (arbitrary-precision h, t = (h W) >> 64, bisect on a list), for its statistics
with the fixed seed -- the device equals the restatement bit for bit (tests/test_mesh_sample_gpu.py), so nothing statistical is ever
run there -- and for the vertex normals of a sphere.  Plus write_glb's NORMAL attribute, which needs no device."""
import bisect
import json
import struct

import numpy as np
import pytest

import mesh_sample_ref as R

MASK = 2 ** 64 - 1

# two triangles of the unit square, and one triangle of three times a square-half's area elsewhere
SCENE_V = np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (5, 0, 0), (8, 0, 0), (5, 1, 0)], np.float32)
SCENE_F = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6]], np.int32)
SCENE_C = np.array([0xFF0000FF, 0xFF00FF00, 0xFFFF0000, 0x80FFFFFF, 0x00000000, 0xFFFFFFFF, 0x7F7F7F7F], np.uint32)
N = 65536


def _h(c, seed):
    z = (seed + (c + 1) * 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def _loop(vertices, rgba, faces, n, seed):
    """the rule sample by sample: Python integers for everything integer, numpy float64 scalars for the five fp64 operations"""
    fr = R.face_frames(vertices, faces)
    cum, W = [int(x) for x in fr["cum"]], fr["W"]
    v = np.asarray(vertices, np.float32).astype(np.float64)
    pts, fidx, col = np.zeros((n, 3), np.float32), np.zeros(n, np.int32), np.zeros(n, np.uint32)
    for k in range(n):
        t = (_h(3 * k, seed) * W) >> 64
        f = bisect.bisect_right(cum, t)
        a, b = _h(3 * k + 1, seed) >> 40, _h(3 * k + 2, seed) >> 40
        if a + b > 2 ** 24:
            a, b = 2 ** 24 - a, 2 ** 24 - b
        ia, ib, ic = (int(x) for x in faces[f])
        ua, ub = np.float64(a) / np.float64(2 ** 24), np.float64(b) / np.float64(2 ** 24)
        for x in range(3):
            e1, e2 = v[ib, x] - v[ia, x], v[ic, x] - v[ia, x]
            pts[k, x] = np.float32(v[ia, x] + (ua * e1 + ub * e2))
        fidx[k] = f
        if rgba is not None:
            p = 0
            for byte in range(4):
                ca, cb, cc = ((int(rgba[i]) >> (8 * byte)) & 255 for i in (ia, ib, ic))
                p |= ((ca * (2 ** 24 - a - b) + cb * a + cc * b + 2 ** 23) >> 24) << (8 * byte)
            col[k] = p
    return pts, fidx, col


@pytest.fixture(scope="module")
def drawn():
    return R.sample(SCENE_V, SCENE_C, SCENE_F, N, seed=0)


def test_the_generator_and_umulhi_equal_python_integers():
    c = np.array([0, 1, 2, 3 * (N - 1), 2 ** 40, 2 ** 63, MASK], np.uint64)
    for seed in (0, 1, 12345, MASK, -1):
        assert [int(x) for x in R.h(c, seed)] == [_h(int(x), seed & MASK) for x in c]
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.integers(0, 2 ** 64, 500, dtype=np.uint64), np.array([0, 1, MASK, 2 ** 32, 2 ** 32 - 1], np.uint64)])
    y = np.concatenate([rng.integers(0, 2 ** 63, 500, dtype=np.uint64), np.array([MASK, MASK, MASK, 2 ** 32, 2 ** 32 + 1], np.uint64)])
    assert [int(v) for v in R.umulhi64(x, y)] == [(int(a) * int(b)) >> 64 for a, b in zip(x, y)]


def test_the_frames_of_the_three_face_scene():
    fr = R.face_frames(SCENE_V, SCENE_F)
    assert fr["d"].tolist() == [1.0, 1.0, 3.0] and fr["dmax"] == 3.0
    assert fr["w"].tolist() == [2 ** 32 // 3, 2 ** 32 // 3, 2 ** 32] and fr["W"] == 2 * (2 ** 32 // 3) + 2 ** 32
    assert fr["cum"].dtype == np.uint64 and fr["cum"].tolist() == [2 ** 32 // 3, 2 * (2 ** 32 // 3), fr["W"]]
    assert np.array_equal(fr["face_normals"], np.array([[0, 0, 1]] * 3, np.float32))
    assert abs(fr["area"] - 2.5) < 3 * 3.0 * 2.0 ** -33                            # the quantised area: short by less than F dmax 2^-33
    assert fr["area"] <= 2.5


def test_the_restatement_equals_the_sample_by_sample_loop(drawn):
    n = 4096
    pts, fidx, col = _loop(SCENE_V, SCENE_C, SCENE_F, n, 0)
    assert np.array_equal(drawn["face_index"][:n], fidx)                          # (the first n of a longer draw are the shorter draw)
    assert np.array_equal(drawn["points"][:n].view(np.uint32), pts.view(np.uint32))
    assert np.array_equal(drawn["rgba"][:n], col)
    # another seed, a mesh whose faces differ by 2^20 in area, faces that can never be drawn in between
    rng = np.random.default_rng(3)
    v = rng.normal(size=(40, 3)).astype(np.float32)
    v[30:33] = v[0] + rng.normal(size=(3, 3)).astype(np.float32) * np.float32(2.0 ** -10)
    f = rng.integers(0, 30, (60, 3)).astype(np.int32)
    f[7], f[8], f[9], f[59] = (30, 31, 32), (1, 1, 2), (-1, 2, 3), (3, 40, 2)
    c = rng.integers(0, 2 ** 32, 40, dtype=np.uint32)
    got = R.sample(v, c, f, 2000, seed=12345)
    pts, fidx, col = _loop(v, c, f, 2000, 12345)
    assert np.array_equal(got["face_index"], fidx) and np.array_equal(got["points"].view(np.uint32), pts.view(np.uint32))
    assert np.array_equal(got["rgba"], col)
    w = R.face_frames(v, f)["w"]
    assert w[8] == w[9] == w[59] == 0 and 0 < w[7] < 2 ** 16 and not np.isin(got["face_index"], [8, 9, 59]).any()


def test_the_face_counts_follow_the_areas(drawn):
    counts = np.bincount(drawn["face_index"], minlength=3)
    p = np.array([0.2, 0.2, 0.6])
    z = (counts - N * p) / np.sqrt(N * p * (1 - p))
    print("counts", counts.tolist(), "z", z.round(2).tolist())
    assert counts.sum() == N and (np.abs(z) <= 4).all()                            # measured: 12916 / 13059 / 39561, |z| <= 1.91


def test_the_samples_of_the_square_are_uniform(drawn):
    sq = drawn["points"][drawn["face_index"] < 2]
    cell = np.minimum((sq[:, :2] * 16).astype(np.int64), 15)
    counts = np.bincount(cell[:, 1] * 16 + cell[:, 0], minlength=256)
    expect = len(sq) / 256.0
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    print("chi-square over 16 x 16 cells of %d samples: %.1f" % (len(sq), chi2))
    assert chi2 <= 340.0                                                           # 255 degrees of freedom, about the 99.9 % point; measured 226.9


def test_every_point_lies_in_its_triangle(drawn):
    p, f = drawn["points"].astype(np.float64), drawn["face_index"]
    assert (p[:, 2] == 0).all()                                                    # the plane
    tri = SCENE_V[SCENE_F[f]].astype(np.float64)                                    # [n, 3, 3]
    assert (p >= tri.min(1)).all() and (p <= tri.max(1)).all()                      # the bounding box
    # inside the triangle itself: the three edge functions are non-negative (counter-clockwise faces), up to the fp32 narrowing
    for i in range(3):
        a, b = tri[:, i, :2], tri[:, (i + 1) % 3, :2]
        side = (b[:, 0] - a[:, 0]) * (p[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (p[:, 0] - a[:, 0])
        assert (side >= -1e-6).all()
    assert np.array_equal(drawn["normals"], np.array([[0, 0, 1]], np.float32).repeat(N, 0))
    # the colours stay between the corners' per byte
    c = SCENE_C[SCENE_F[f]]
    for byte in range(4):
        b3 = (c >> np.uint32(8 * byte)) & np.uint32(255)
        got = (drawn["rgba"] >> np.uint32(8 * byte)) & np.uint32(255)
        assert (got >= b3.min(1)).all() and (got <= b3.max(1)).all()


@pytest.mark.parametrize("seed", [1, 12345])
def test_other_seeds_pass_the_same_bars(seed):
    s = R.sample(SCENE_V, None, SCENE_F, N, seed=seed)
    counts = np.bincount(s["face_index"], minlength=3)
    p = np.array([0.2, 0.2, 0.6])
    assert (np.abs((counts - N * p) / np.sqrt(N * p * (1 - p))) <= 4).all()
    sq = s["points"][s["face_index"] < 2]
    cell = np.minimum((sq[:, :2] * 16).astype(np.int64), 15)
    counts = np.bincount(cell[:, 1] * 16 + cell[:, 0], minlength=256)
    assert float(((counts - len(sq) / 256.0) ** 2 / (len(sq) / 256.0)).sum()) <= 340.0
    assert s["rgba"] is None


def test_nothing_to_sample_raises_and_zero_samples_are_empty():
    with pytest.raises(ValueError, match="no area to sample"):
        R.sample(SCENE_V, None, np.zeros((0, 3), np.int32), 5)
    with pytest.raises(ValueError, match="no area to sample"):
        R.sample(SCENE_V, None, np.array([[0, 0, 1], [0, 1, 9]], np.int32), 5)
    s = R.sample(SCENE_V, SCENE_C, SCENE_F, 0)
    assert s["points"].shape == (0, 3) and s["normals"].shape == (0, 3) and s["rgba"].shape == (0,) and s["face_index"].dtype == np.int32
    fr = R.face_frames(SCENE_V, np.zeros((0, 3), np.int32))
    assert fr["W"] == 0 and fr["dmax"] == 0 and fr["area"] == 0


def uv_sphere(nlat, nlon):
    """a unit sphere of nlat bands and nlon sectors, outward faces"""
    vs = [(0.0, 0.0, 1.0)]
    for i in range(1, nlat):
        th = np.pi * i / nlat
        vs += [(np.sin(th) * np.cos(2 * np.pi * j / nlon), np.sin(th) * np.sin(2 * np.pi * j / nlon), np.cos(th)) for j in range(nlon)]
    vs.append((0.0, 0.0, -1.0))
    fs = [(0, 1 + j, 1 + (j + 1) % nlon) for j in range(nlon)]
    for i in range(nlat - 2):
        for j in range(nlon):
            a, b = 1 + i * nlon + j, 1 + i * nlon + (j + 1) % nlon
            fs += [(a, a + nlon, b), (b, a + nlon, b + nlon)]
    last, base = len(vs) - 1, 1 + (nlat - 2) * nlon
    fs += [(last, base + (j + 1) % nlon, base + j) for j in range(nlon)]
    return np.array(vs, np.float32), np.array(fs, np.int32)


def test_vertex_normals_of_a_sphere_point_outwards():
    """The angle between the area-weighted vertex normal and the radial direction on a UV sphere of 24 x 48: measured maximum
    1.2678 degrees (next to the poles, where the triangles of a band are most unequal); asserted at twice that.  It is a property
    of the tessellation and of area weighting, not of the arithmetic."""
    v, f = uv_sphere(24, 48)
    n = R.vertex_normals(v, f)
    assert n.dtype == np.float32 and n.shape == v.shape
    cosang = (n.astype(np.float64) * v / np.linalg.norm(v.astype(np.float64), axis=1, keepdims=True)).sum(1)
    angle = np.degrees(np.arccos(np.clip(cosang, -1, 1)))
    print("largest angle to the radial direction: %.4f degrees" % angle.max())
    assert angle.max() <= 2 * 1.2678
    assert np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1).max() < 1e-6
    # the sums are integers: any order of the faces gives the same bits; a vertex no face names gets zeros
    perm = np.random.default_rng(1).permutation(len(f))
    assert np.array_equal(R.vertex_normals(v, f[perm]).view(np.uint32), n.view(np.uint32))
    lonely = R.vertex_normals(np.concatenate([v, [[9, 9, 9]]]).astype(np.float32), f)
    assert np.array_equal(lonely[:-1].view(np.uint32), n.view(np.uint32)) and (lonely[-1] == 0).all()
    # sums against a face-by-face loop over Python integers
    s = R.vertex_sums(v, f)
    fr = R.face_frames(v, f)
    want = [[0, 0, 0] for _ in range(len(v))]
    for face, nn in zip(f.tolist(), fr["n"]):
        q = [int(np.rint(x / fr["dmax"] * 1073741824.0)) for x in nn]
        for i in face:
            for c in range(3):
                want[i][c] += q[c]
    assert s.tolist() == want


# ------------------------------------------------------------------------------------------------ write_glb(normals=)
def _glb(path):
    raw = open(path, "rb").read()
    magic, version, total = struct.unpack_from("<4sII", raw, 0)
    jlen, jtag = struct.unpack_from("<I4s", raw, 12)
    doc = json.loads(raw[20:20 + jlen])
    blen, btag = struct.unpack_from("<I4s", raw, 20 + jlen)
    assert magic == b"glTF" and version == 2 and total == len(raw) and jtag == b"JSON" and btag == b"BIN\0"
    return doc, raw[28 + jlen:28 + jlen + blen]


def test_write_glb_without_normals_is_byte_identical_and_with_them_round_trips(tmp_path):
    from spann3r_amd import mesh as M
    v, f = uv_sphere(6, 8)
    c = (np.arange(len(v) * 4) % 251).astype(np.uint8).reshape(-1, 4)
    n = R.vertex_normals(v, f)
    a, b, w, cloud = (str(tmp_path / x) for x in ("a.glb", "b.glb", "n.glb", "cloud.glb"))
    M.write_glb(a, v, c, f)
    M.write_glb(b, v, c, f, normals=None)
    assert open(a, "rb").read() == open(b, "rb").read()
    doc0, _ = _glb(a)
    assert "NORMAL" not in doc0["meshes"][0]["primitives"][0]["attributes"] and len(doc0["accessors"]) == 3
    size = M.write_glb(w, v, c, f, normals=n)
    doc, binary = _glb(w)
    prim = doc["meshes"][0]["primitives"][0]
    assert size == len(open(w, "rb").read()) and prim["attributes"] == dict(POSITION=0, COLOR_0=1, NORMAL=3) and prim["indices"] == 2
    acc = doc["accessors"][3]
    view = doc["bufferViews"][acc["bufferView"]]
    assert acc == dict(bufferView=3, componentType=5126, count=len(v), type="VEC3")
    assert view == dict(buffer=0, byteOffset=16 * len(v) + 12 * len(f), byteLength=12 * len(v), target=34962)      # appended after the others
    assert doc["bufferViews"][:3] == doc0["bufferViews"] and doc["accessors"][:3] == doc0["accessors"]
    back = np.frombuffer(binary, "<f4", 3 * len(v), view["byteOffset"]).reshape(-1, 3)
    assert np.array_equal(back.view(np.uint32), n.view(np.uint32))
    assert binary[:view["byteOffset"]] == _glb(a)[1][:view["byteOffset"]]
    M.write_glb(cloud, v, c, None, normals=n)                                       # a cloud: the view follows the colours
    doc, binary = _glb(cloud)
    assert doc["meshes"][0]["primitives"][0]["attributes"] == dict(POSITION=0, COLOR_0=1, NORMAL=2)
    assert doc["bufferViews"][2]["byteOffset"] == 16 * len(v)
    with pytest.raises(ValueError, match="normals"):
        M.write_glb(w, v, c, f, normals=n[:-1])
    bad = n.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError, match="non-finite vertex normal"):
        M.write_glb(w, v, c, f, normals=bad)
