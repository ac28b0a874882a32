#!/usr/bin/env python
"""Generate tests/golden/mesh_faces.npz: the reference's own pts3d_to_trimesh / cat_meshes (app.py) on seeded inputs.

    python tests/golden/make_golden_mesh.py --reference <checkout of the reference>

app.py cannot be imported (gradio, trimesh, and a model load at import time).  The script parses it at generation time, takes the
two function definitions out of the module's syntax tree UNMODIFIED and runs them with numpy alone; none of the reference's text
is kept here.  Cases (keys <case>_img / _pts / _valid as inputs, <case>_vertices / _faces / _face_colors as the reference's output):

  c2x2_none, c2x2_tl, c2x2_tr, c2x2_bl, c2x2_br   a 2 x 2 pointmap with no / each single corner invalid
  c5x7                                            5 x 7 with a random mask
  c9x13x3                                         three 9 x 13 frames through cat_meshes: random mask, fully masked, fully valid
                                                  (inputs stacked [3, ...]; a frame's face indices are shifted by cat_meshes)"""
import argparse
import ast
import os

import numpy as np

SEED = 0


def reference_functions(reference):
    path = os.path.join(reference, "app.py")
    tree = ast.parse(open(path).read(), filename=path)
    wanted = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ("pts3d_to_trimesh", "cat_meshes")]
    assert sorted(n.name for n in wanted) == ["cat_meshes", "pts3d_to_trimesh"], [n.name for n in wanted]
    ns = {"np": np}
    exec(compile(ast.Module(body=wanted, type_ignores=[]), path, "exec"), ns)
    return ns["pts3d_to_trimesh"], ns["cat_meshes"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("SPANN3R_REFERENCE"), required="SPANN3R_REFERENCE" not in os.environ)
    args = ap.parse_args()
    to_mesh, cat = reference_functions(args.reference)
    rng = np.random.default_rng(SEED)
    out = {}

    def frame(h, w):
        return rng.random((h, w, 3), dtype=np.float32), rng.standard_normal((h, w, 3)).astype(np.float32)

    def put(name, img, pts, valid, mesh):
        out.update({name + "_img": img, name + "_pts": pts, name + "_valid": valid, name + "_vertices": mesh["vertices"],
                    name + "_faces": mesh["faces"], name + "_face_colors": mesh["face_colors"]})

    for name, corner in (("none", None), ("tl", (0, 0)), ("tr", (0, 1)), ("bl", (1, 0)), ("br", (1, 1))):
        img, pts = frame(2, 2)
        valid = np.ones((2, 2), bool)
        if corner is not None:
            valid[corner] = False
        put("c2x2_" + name, img, pts, valid, to_mesh(img, pts, valid))
    img, pts = frame(5, 7)
    valid = rng.random((5, 7)) < 0.7
    put("c5x7", img, pts, valid, to_mesh(img, pts, valid))
    frames = [frame(9, 13) for _ in range(3)]
    valids = [rng.random((9, 13)) < 0.7, np.zeros((9, 13), bool), np.ones((9, 13), bool)]
    mesh = cat([to_mesh(i, p, v) for (i, p), v in zip(frames, valids)])
    put("c9x13x3", np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames]), np.stack(valids), mesh)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mesh_faces.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", {k: out[k].shape for k in out if k.endswith("_faces")})


if __name__ == "__main__":
    main()
