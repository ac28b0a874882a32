"""Float64 numpy restatement of the point rasteriser's rule (include/spann3r_hip.h, "Headless point-cloud rendering"): projection,
footprint, z-test with the lowest-index tie rule, resolve and rgba packing.  It is the pin of spann3r_amd.vis in tests/test_vis.py;
Open3D, whose window the reference renders through, is not available, so this is a restatement and not Open3D's output.

The z-test runs np.minimum.at on the same 64-bit keys as the device, (depth rank << 32) | index, but the rank is the position of
the float64 depth among the sorted distinct float64 depths, not an fp32 bit pattern."""
import numpy as np


class Cam:
    """R [3, 3] and t [3] world-to-camera, intrinsics, image size, z_near, point_size: the fields of sp3_render_cam, float64"""

    def __init__(self, R, t, fx, fy, cx, cy, width, height, z_near=0.0, point_size=1):
        self.R, self.t = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
        self.fx, self.fy, self.cx, self.cy = float(fx), float(fy), float(cx), float(cy)
        self.width, self.height, self.z_near, self.point_size = int(width), int(height), float(z_near), int(point_size)


def project(pts, cam):
    """-> (u, v, z, ok) float64 per point; ok = finite and z > z_near (u, v are nan where not ok)"""
    X = np.asarray(pts, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        Xc = X @ cam.R.T + cam.t
        ok = np.isfinite(X).all(1) & np.isfinite(Xc).all(1)
        ok &= np.where(ok, Xc[:, 2], 0.0) > cam.z_near
        z = np.where(ok, Xc[:, 2], 1.0)
        u = np.where(ok, cam.fx * Xc[:, 0] / z + cam.cx, np.nan)
        v = np.where(ok, cam.fy * Xc[:, 1] / z + cam.cy, np.nan)
    return u, v, np.where(ok, Xc[:, 2], np.nan), ok


def boundary_distance(pts, cam):
    """per drawn point, the distance in pixels of its float64 projection from the nearest rounding boundary (k + 0.5); inf where culled"""
    u, v, _, ok = project(pts, cam)
    d = np.full(len(u), np.inf)
    for c in (u, v):
        fr = c[ok] + 0.5 - np.floor(c[ok] + 0.5)
        d[ok] = np.minimum(d[ok], np.minimum(fr, 1 - fr))
    return d


def render(pts, cam, keep=None):
    """-> (index int64 [H, W] (-1: empty), depth float64 [H, W] (+inf: empty)).  pts [n, 3]; the index is the row of pts; keep
    (bool [n], optional) drops points without renumbering the rest."""
    u, v, z, ok = project(pts, cam)
    if keep is not None:
        ok = ok & np.asarray(keep, bool).reshape(-1)
    H, W, ps = cam.height, cam.width, cam.point_size
    big = 1 << 40                                                # beyond any footprint: keeps the integer conversion defined
    with np.errstate(all="ignore"):
        px = np.where(ok, np.clip(np.floor(u + 0.5), -big, big), -big).astype(np.int64)
        py = np.where(ok, np.clip(np.floor(v + 0.5), -big, big), -big).astype(np.int64)
    levels = np.unique(z[ok])
    rank = np.searchsorted(levels, np.where(ok, z, 0.0)).astype(np.uint64)
    keys = np.full(H * W, np.iinfo(np.uint64).max, np.uint64)
    idx = np.arange(len(u), dtype=np.uint64)
    key = (rank << np.uint64(32)) | idx
    off = (ps - 1) // 2
    for dy in range(ps):
        for dx in range(ps):
            x, y = px - off + dx, py - off + dy
            m = ok & (x >= 0) & (x < W) & (y >= 0) & (y < H)
            np.minimum.at(keys, (y[m] * W + x[m]), key[m])
    empty = keys == np.iinfo(np.uint64).max
    index = np.where(empty, -1, (keys & np.uint64(0xffffffff)).astype(np.int64))
    depth = np.where(empty, np.inf, z[np.where(empty, 0, index)] if len(u) else np.inf)
    return index.reshape(H, W), depth.reshape(H, W)


def pack_rgba8(colors):
    """uint8 [n, 3] = clamp(floor(c * 255 + 0.5), 0, 255) of floats in [0, 1]"""
    c = np.asarray(colors, np.float64).reshape(-1, 3)
    return np.clip(np.floor(c * 255 + 0.5), 0, 255).astype(np.uint8)


def resolve(index, colors, background=(0, 0, 0)):
    """uint8 [H, W, 3]: the packed colour of the winning point, the packed background where empty"""
    rgb8 = pack_rgba8(colors)
    bg = pack_rgba8(np.asarray(background, np.float64)[None])[0]
    out = np.empty(index.shape + (3,), np.uint8)
    out[...] = bg
    m = index >= 0
    out[m] = rgb8[index[m]]
    return out
