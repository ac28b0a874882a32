"""spann3r_amd.mesh without a GPU: the GLB writer parsed back by a reader kept here, argument errors, and the numpy restatement of
the face rule (tests/mesh_ref.py) against the reference's own output (tests/golden/mesh_faces.npz)."""
import ctypes
import json
import struct

import numpy as np
import pytest
import torch

from conftest import load_golden
import mesh_ref as MR
from spann3r_amd import mesh as M

CASES_1 = ["c2x2_none", "c2x2_tl", "c2x2_tr", "c2x2_bl", "c2x2_br", "c5x7"]
COMPONENT = {5126: ("<f4", 4), 5121: ("u1", 1), 5125: ("<u4", 4)}
WIDTH = {"SCALAR": 1, "VEC3": 3, "VEC4": 4}


def read_glb(path):
    """A strict reader of what write_glb promises -> dict(json, positions, colors, indices or None, mode, length).  Asserts the
    container rules on the way: magic, version, total length, chunk order, lengths and padding, one buffer, aligned buffer views."""
    data = open(path, "rb").read()
    magic, version, total = struct.unpack_from("<4sII", data, 0)
    assert magic == b"glTF" and version == 2 and total == len(data) and total % 4 == 0
    n_json, kind = struct.unpack_from("<I4s", data, 12)
    assert kind == b"JSON" and n_json % 4 == 0
    text = data[20:20 + n_json]
    doc = json.loads(text.decode())
    assert text.rstrip(b" ") == json.dumps(doc, separators=(",", ":")).encode()            # padded with spaces only
    n_bin, kind = struct.unpack_from("<I4s", data, 20 + n_json)
    assert kind == b"BIN\0" and n_bin % 4 == 0 and 28 + n_json + n_bin == total
    binary = data[28 + n_json:]
    assert doc["asset"]["version"] == "2.0" and len(doc["buffers"]) == 1
    assert doc["buffers"][0]["byteLength"] <= n_bin < doc["buffers"][0]["byteLength"] + 4
    assert set(binary[doc["buffers"][0]["byteLength"]:]) <= {0}
    arrays = []
    for acc in doc["accessors"]:
        view = doc["bufferViews"][acc["bufferView"]]
        dt, size = COMPONENT[acc["componentType"]]
        assert view["buffer"] == 0 and view["byteOffset"] % 4 == 0 and view["byteLength"] % 4 == 0
        assert view["byteOffset"] + view["byteLength"] <= doc["buffers"][0]["byteLength"]
        assert view["byteLength"] == acc["count"] * WIDTH[acc["type"]] * size and acc["count"] >= 1
        arrays.append(np.frombuffer(binary, dt, acc["count"] * WIDTH[acc["type"]], view["byteOffset"]).reshape(acc["count"], -1))
    (prim,) = doc["meshes"][0]["primitives"]
    pos_acc, col_acc = doc["accessors"][prim["attributes"]["POSITION"]], doc["accessors"][prim["attributes"]["COLOR_0"]]
    assert pos_acc["componentType"] == 5126 and pos_acc["type"] == "VEC3"
    assert col_acc["componentType"] == 5121 and col_acc["type"] == "VEC4" and col_acc["normalized"] is True
    pos, col = arrays[prim["attributes"]["POSITION"]], arrays[prim["attributes"]["COLOR_0"]]
    assert len(pos) == len(col)
    assert pos_acc["min"] == [float(x) for x in pos.min(0)] and pos_acc["max"] == [float(x) for x in pos.max(0)]
    idx = None
    if "indices" in prim:
        acc = doc["accessors"][prim["indices"]]
        assert acc["componentType"] == 5125 and acc["type"] == "SCALAR" and acc["count"] % 3 == 0
        assert doc["bufferViews"][acc["bufferView"]]["target"] == 34963
        idx = arrays[prim["indices"]].reshape(-1, 3)
        assert idx.max() < len(pos)
        assert prim["mode"] == 4 and doc["materials"][prim["material"]]["doubleSided"] is True
    else:
        assert prim["mode"] == 0
    assert doc["scenes"][doc["scene"]]["nodes"] == [0] and doc["nodes"][0]["mesh"] == 0
    return dict(json=doc, positions=pos, colors=col, indices=idx, mode=prim["mode"], length=total)


def _mesh_inputs(v=7, f=5, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((v, 3)).astype(np.float32), rng.integers(0, 256, (v, 4), dtype=np.uint8),
            rng.integers(0, v, (f, 3)).astype(np.int32))


@pytest.mark.parametrize("v,f", [(7, 5), (1, 1), (258, 511)])
def test_write_glb_mesh_round_trip(tmp_path, v, f):
    pos, col, faces = _mesh_inputs(v, f)
    path = str(tmp_path / "m.glb")
    size = M.write_glb(path, pos, col, faces)
    g = read_glb(path)
    assert g["length"] == size and g["mode"] == 4
    assert np.array_equal(g["positions"], pos) and np.array_equal(g["colors"], col) and np.array_equal(g["indices"], faces)
    assert g["json"]["accessors"][2]["count"] == 3 * f and g["json"]["accessors"][0]["count"] == v


def test_write_glb_points_rgb_and_tensors(tmp_path):
    """no faces: POINTS; uint8 [V, 3] colours get alpha 255; CPU tensors are accepted by the writer (it is host code)"""
    pos, col, _ = _mesh_inputs(9)
    path = str(tmp_path / "p.glb")
    M.write_glb(path, torch.from_numpy(pos), torch.from_numpy(col[:, :3].copy()))
    g = read_glb(path)
    assert g["mode"] == 0 and g["indices"] is None and "materials" not in g["json"]
    assert np.array_equal(g["positions"], pos) and np.array_equal(g["colors"][:, :3], col[:, :3]) and (g["colors"][:, 3] == 255).all()
    # odd colour byte counts cannot unalign a view: 9 * 4 bytes of colours, 9 * 12 of positions
    assert [v["byteOffset"] for v in g["json"]["bufferViews"]] == [0, 108]


def test_write_glb_given_bounds(tmp_path):
    pos, col, faces = _mesh_inputs()
    M.write_glb(str(tmp_path / "b.glb"), pos, col, faces, bounds=np.stack([pos.min(0), pos.max(0)]))
    read_glb(str(tmp_path / "b.glb"))


def test_write_glb_argument_errors(tmp_path):
    pos, col, faces = _mesh_inputs()
    path = str(tmp_path / "e.glb")
    with pytest.raises(ValueError, match="mismatched lengths"):
        M.write_glb(path, pos, col[:-1], faces)
    with pytest.raises(ValueError, match="face index"):
        M.write_glb(path, pos, col, faces + 7)
    with pytest.raises(ValueError, match="uint8"):
        M.write_glb(path, pos, col.astype(np.float32), faces)
    with pytest.raises(ValueError, match="V >= 1"):
        M.write_glb(path, pos[:0], col[:0])
    with pytest.raises(ValueError, match="non-finite"):
        M.write_glb(path, pos * np.float32("inf"), col)
    with pytest.raises(ValueError, match=r"\[F, 3\]"):
        M.write_glb(path, pos, col, faces.reshape(-1))


def test_device_functions_refuse_cpu_tensors():
    img, pts, conf = torch.rand(4, 5, 3), torch.rand(4, 5, 3), torch.rand(4, 5) + 1
    with pytest.raises(RuntimeError, match="no CPU path"):
        M.pts3d_to_mesh(img, pts)
    with pytest.raises(RuntimeError, match="no CPU path"):
        M.scene_mesh(pts[None], img[None], conf[None], 1e-3)
    with pytest.raises(TypeError, match="CUDA tensor"):
        M.pts3d_to_mesh(img.numpy(), pts.numpy())
    with pytest.raises(ValueError, match="no meshes"):
        M.cat_meshes([])
    from spann3r_amd import vis
    with pytest.raises(RuntimeError, match="no CPU path"):
        vis.render_frames(pts[None], img[None], None, surface=True)


def test_library_validates_mesh_arguments_without_a_gpu():
    from spann3r_amd import lib
    l = lib.load()
    one = ctypes.c_void_p(16)
    assert l.sp3_mesh_faces(one, one, 0.0, None, 1, 4, 4, 1, one, one, one, one, None) != 0
    assert b"valid or conf, not both" in l.sp3_last_error()
    assert l.sp3_mesh_faces(None, None, 0.0, None, 1, 4, 4, 2, one, one, one, one, None) != 0
    assert b"both_windings" in l.sp3_last_error()
    assert l.sp3_mesh_faces(None, None, 0.0, None, 1 << 20, 1 << 10, 1 << 10, 1, one, one, one, one, None) != 0
    assert b"2^31" in l.sp3_last_error()
    assert l.sp3_mesh_faces(None, None, 0.0, None, 0, 4, 4, 1, None, None, None, None, None) == 0          # t = 0: a no-op
    cam = lib.RenderCam((ctypes.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1), (ctypes.c_float * 3)(), 1, 1, 0, 0, 8, 8, 0.0, 1)
    assert l.sp3_render_tris(one, 3, one, None, 1, None, 0, ctypes.byref(cam), 0, one, None, None) != 0
    assert b"max_bbox_px" in l.sp3_last_error()
    assert l.sp3_render_tris(one, 3, one, None, 1, None, (1 << 32) - 3, ctypes.byref(cam), 16, one, None, None) != 0
    assert b"index overflow" in l.sp3_last_error()
    assert l.sp3_render_tris(None, 0, None, None, 0, None, 0, ctypes.byref(cam), 16, None, None, None) == 0      # no faces: a no-op
    assert l.sp3_mesh_compact_vertices(one, None, 4, one, 1, one, None, 0.0, 1.0, None, one, one, None, one, one, None) != 0
    assert b"with faces" in l.sp3_last_error()
    assert l.sp3_mesh_compact_vertices(None, None, 0, None, 0, None, None, 0.0, 1.0, None, None, None, None, None, None, None) == 0
    assert l.sp3_mesh_faces_ws_bytes(3, 64, 80) >= 3 * 64 * 80 and l.sp3_mesh_vertices_ws_bytes(1000) >= 4000


@pytest.mark.parametrize("case", CASES_1)
def test_restatement_matches_the_reference_single_frame(case):
    g = load_golden("mesh_faces.npz")
    faces, colour, counts = MR.faces_ref(g[case + "_valid"][None])
    assert np.array_equal(faces, g[case + "_faces"]) and faces.dtype == g[case + "_faces"].dtype
    assert np.array_equal(g[case + "_img"].reshape(-1, 3)[colour], g[case + "_face_colors"])
    assert counts[0] == len(faces) == sum(counts[1:])
    fwd, col_fwd, _ = MR.faces_ref(g[case + "_valid"][None], both_windings=False)
    c = counts[1:]
    rows = np.r_[np.arange(c[0]), c[0] + c[1] + np.arange(c[2])].astype(int)
    assert np.array_equal(fwd, faces[rows]) and np.array_equal(col_fwd, colour[rows])


def test_restatement_matches_the_reference_cat_meshes():
    g = load_golden("mesh_faces.npz")
    faces, colour, counts = MR.faces_ref(g["c9x13x3_valid"])
    assert np.array_equal(faces, g["c9x13x3_faces"])
    assert np.array_equal(g["c9x13x3_img"].reshape(-1, 3)[colour], g["c9x13x3_face_colors"])
    assert np.array_equal(g["c9x13x3_pts"].reshape(-1, 3), g["c9x13x3_vertices"])
    assert counts[5:9] == [0, 0, 0, 0] and counts[9:13] == [96] * 4             # the fully masked and the fully valid frame


def test_scene_transform_is_the_stated_diagonal():
    """app.py:165-167 with scipy's Rotation, as the docstring of scene_mesh states it"""
    from scipy.spatial.transform import Rotation
    opengl = np.diag([1.0, -1.0, -1.0, 1.0])
    rot = np.eye(4)
    rot[:3, :3] = Rotation.from_euler("y", np.deg2rad(180)).as_matrix()
    assert np.allclose(np.linalg.inv(opengl @ rot), M.TRANSFORM, atol=1e-15) and M.SCALE == 10.0
