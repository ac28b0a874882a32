"""Generate tests/golden/eval_metrics.npz: the reference's own reconstruction metrics and a float64 oracle of ICP / normals on
seeded clouds (tests/eval_ref.py builds them), plus the measured quantities the tolerances of tests/test_evaluate.py rest on.

    python tests/golden/make_golden_eval.py --reference <checkout of the reference>

Needs scipy and the reference checkout: spann3r/tools/eval_recon.py is loaded from it UNMODIFIED and run on the main cloud pair.
Open3D is not required (and its parity is not pinned): ICP and the normals are tests/eval_ref.py's float64 restatement with
scipy's cKDTree as the neighbour search.  The file is written with fixed zip timestamps: a re-run reproduces it bit for bit."""
import argparse
import importlib.util
import io
import os
import sys
import zipfile

import numpy as np
from scipy.spatial import cKDTree

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import eval_ref as R  # noqa: E402


def tree_nn(query, ref):
    d, i = cKDTree(np.asarray(ref, np.float64)).query(np.asarray(query, np.float64))
    return d, i


def nn_fp32(query, ref):
    d, i = R.nn_brute(query, ref, np.float32)
    return d.astype(np.float64), i


def near_ties(query, ref, bound):
    """queries whose best and second-best float64 distances differ by less than twice the fp32 bound"""
    d, _ = cKDTree(np.asarray(ref, np.float64)).query(np.asarray(query, np.float64), k=2)
    return int(np.sum(d[:, 1] - d[:, 0] < 2 * bound(d[:, 0])))


def median_window(dots, m):
    """the reference's order statistics m ranks either side of the median"""
    s = np.sort(dots)
    n = len(s)
    return np.array([s[max((n - 1) // 2 - m, 0)], s[min(n // 2 + m, n - 1)]])


def icp_case(src, tgt, max_dist, bound):
    T, fit, rmse, it, d = R.icp(src, tgt, max_dist, nn=tree_nn)
    T32, fit32, _, it32, _ = R.icp(src, tgt, max_dist, nn=nn_fp32, fp32_points=True)
    border = int(np.sum(np.abs(d - max_dist) <= bound(d)))
    return {"T": T, "fitness": fit, "rmse": rmse, "iterations": it, "borderline": border,
            "rot_dev": R.rot_angle(T32[:3, :3], T[:3, :3]), "trans_dev": float(np.linalg.norm(T32[:3, 3] - T[:3, 3])),
            "iterations_fp32": it32, "fitness_fp32": fit32}


def write_npz(path, arrays):
    """np.savez_compressed with every zip timestamp fixed"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("SPANN3R_REFERENCE"), required="SPANN3R_REFERENCE" not in os.environ)
    ap.add_argument("--out", default=os.path.join(HERE, "eval_metrics.npz"))
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location("eval_recon", os.path.join(args.reference, "spann3r", "tools", "eval_recon.py"))
    E = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(E)

    out = {}
    gt, rec = R.main_pair()
    mc = R.max_coord(gt, rec)

    def bound(d):
        return R.dist_bound(d, mc)

    gt64, rec64 = gt.astype(np.float64), rec.astype(np.float64)
    d_acc, i_acc = tree_nn(rec64, gt64)
    d_comp, i_comp = tree_nn(gt64, rec64)
    # brute force in float64 and the KD-tree agree on this pair (what lets tests/eval_ref.py stand in for scipy)
    db, ib = R.nn_brute(rec64, gt64)
    assert np.abs(db - d_acc).max() <= 1e-12 and np.array_equal(ib, i_acc)
    db, ib = R.nn_brute(gt64, rec64)
    assert np.abs(db - d_comp).max() <= 1e-12 and np.array_equal(ib, i_comp)

    # oracle normals: k-NN (cKDTree) + PCA in float64; the same with search and covariance in fp32
    def normals(p):
        p64 = p.astype(np.float64)
        _, nbr = cKDTree(p64).query(p64, k=30)
        n64, w = R.pca_normals(p64, nbr)
        _, nbr32 = R.knn_brute(p, p, 30, np.float32)
        n32, _ = R.pca_normals(p, nbr32, np.float32)
        dev = float(np.max(1.0 - np.abs(np.sum(n32.astype(np.float64) * n64, -1))))
        gap = float(np.min((w[:, 1] - w[:, 0]) / w[:, 2]))
        return n64, dev, gap

    gt_n, dev_gt, gap_gt = normals(gt)
    rec_n, _, _ = normals(rec)
    # the metrics take fp32 normals (what the device API is given): the float64 oracle of gt stays for the normals test
    gt_n32, rec_n32 = gt_n.astype(np.float32), rec_n.astype(np.float32)
    gt_nm, rec_nm = gt_n32.astype(np.float64), rec_n32.astype(np.float64)

    # the reference's own metrics, with and without normals
    acc4 = E.accuracy(gt64, rec64, gt_nm, rec_nm)
    comp4 = E.completion(gt64, rec64, gt_nm, rec_nm)
    assert tuple(E.accuracy(gt64, rec64)) == tuple(acc4[:2]) and tuple(E.completion(gt64, rec64)) == tuple(comp4[:2])
    ratio = E.completion_ratio(gt64, rec64)
    assert not np.any(np.abs(d_comp - 0.05) <= bound(d_comp)), "a completion distance within the fp32 bound of dist_th"
    assert not np.any(np.abs(d_acc - 0.05) <= bound(d_acc)), "an accuracy distance within the fp32 bound of max_dist = 0.05"
    m_acc, m_comp = near_ties(rec64, gt64, bound), near_ties(gt64, rec64, bound)
    assert m_acc <= 0.005 * len(rec) and m_comp <= 0.005 * len(gt), (m_acc, m_comp)
    dots_acc = np.abs(np.sum(gt_nm[i_acc] * rec_nm, -1))
    dots_comp = np.abs(np.sum(gt_nm * rec_nm[i_comp], -1))
    # numpy fp32 direct differences against the bound (recorded, and it must hold)
    d32, _ = R.nn_brute(rec, gt, np.float32)
    fp32_share = float(np.max(np.abs(d32.astype(np.float64) - d_acc) / bound(d_acc)))
    assert fp32_share < 1.0
    out.update(gt=gt, rec=rec, d_acc=d_acc, d_comp=d_comp, gt_normals=gt_n, rec_normals_f32=rec_n32, ref_accuracy=np.array(acc4, np.float64),
               ref_completion=np.array(comp4, np.float64), ref_completion_ratio=np.float32(ratio), near_ties=np.array([m_acc, m_comp]),
               nc1_median_window=median_window(dots_acc, m_acc), nc2_median_window=median_window(dots_comp, m_comp),
               normals_fp32_dev=dev_gt, normals_min_gap=gap_gt, fp32_share_of_bound=fp32_share)

    # 20 000 x 20 000 uniform: stored cKDTree distances (the clouds are rebuilt from their seed; their sum guards the stream)
    uref, uqry = R.uniform_pair()
    out["uniform_d"], _ = tree_nn(uqry, uref)
    out["uniform_checksum"] = np.array([uref.astype(np.float64).sum(), uqry.astype(np.float64).sum()])

    # ICP: A noise-free, B noisy with 10 % far outliers
    src_a, src_b = R.icp_sources(gt)
    mc_icp = R.max_coord(gt, src_a)            # the matched pairs live inside the cloud: the far outliers of B never match

    def bound_icp(d):
        return R.dist_bound(d, mc_icp)

    for tag, src in (("a", src_a), ("b", src_b)):
        for key, v in icp_case(src, gt64, 0.1, bound_icp).items():
            out["icp_%s_%s" % (tag, key)] = v
    out.update(icp_src_a=src_a, icp_src_b=src_b, icp_motion=R.ICP_MOTION)

    write_npz(args.out, out)
    print(args.out, os.path.getsize(args.out), "bytes")
    for k in sorted(out):
        if np.asarray(out[k]).size <= 16:
            print(" ", k, np.asarray(out[k]).tolist())


if __name__ == "__main__":
    main()
