#!/usr/bin/env python
"""The timed region of the reference's demo.py (lines 81-132) on synthetic frames: build the model, load a state dict,
move only view['img'] to the device, time model.forward(batch), report FPS = len(batch) / seconds (with the device sync the
reference omits).  The real demo.py cannot be imported in this image (cv2 / open3d / torchvision are not installed)."""
import argparse
import math
import time

import torch

from spann3r_amd import Spann3R, FULL, TINY
from spann3r_amd.weights import synth_state_dict, synth_frames


class StreamFuser:
    """--stream --fused --bricks: every frame, as its prediction completes, is posed on its own -- the focal of the first frame
    (estimate_focal_knowing_depth), estimate_poses on that frame alone -- and pushed into a fusion.FusionSession: a brick TSDF volume
    inside --extent (default: a cube of +-4 units around the first camera), tracked with --track.  With --vis the model is ray-cast
    from the frame's camera every --kf_every frames.  Pointmaps without geometry (no checkpoint ships) go through nominal cameras --
    focal = the longer image side, identity poses -- and that is said."""

    def __init__(self, args):
        self.args, self.session, self.focal, self.nominal, self.pictures = args, None, None, False, 0

    def push(self, i, pts, conf, image):
        """pts [1, h, w, 3], conf [1, h, w], image [1, h, w, 3] of frame i"""
        import os
        import numpy as np
        from spann3r_amd import fusion, vis
        from spann3r_amd.postprocess import estimate_focal_knowing_depth, estimate_poses
        args = self.args
        _, h, w, _ = pts.shape
        pp = (w / 2, h / 2)
        if self.session is None:
            self.focal = float(estimate_focal_knowing_depth(pts, torch.tensor(pp), focal_mode="weiszfeld").item())
            self.nominal = not (self.focal > 1e-3 and math.isfinite(self.focal))
            if self.nominal:
                self.focal = float(max(h, w))
                print("degenerate pointmaps: the focal of the first frame came out near 0: fusing through nominal cameras (focal %d, identity poses)"
                      % max(h, w))
        pose = np.eye(4) if self.nominal else np.asarray(estimate_poses(pts, self.focal, pp)[0][0], np.float64)
        if self.session is None:
            lo, hi = (pose[:3, 3] - 4.0, pose[:3, 3] + 4.0) if args.extent is None else (args.extent[:3], args.extent[3:])
            self.session = fusion.FusionSession(args.voxel_size, (lo, hi), trunc_voxels=args.trunc_voxels, track=args.track)
        K = np.array([[self.focal, 0, pp[0]], [0, self.focal, pp[1]], [0, 0, 1]], np.float64)
        used, _ = self.session.push(pts[0], K, pose, (conf[0] - 1) / conf[0] > args.conf_thresh, image[0])
        if args.vis and i % args.kf_every == 0:
            rc = self.session.raycast(K, used[None], (h, w))
            view = rc["vertices"][0] - torch.from_numpy(used[:3, 3]).to(rc["vertices"])
            view = view / view.norm(dim=-1, keepdim=True).clamp_min(1e-30)
            shade = (-(rc["normals"][0] * view).sum(-1)).clamp_min(0.0) * (rc["depth"][0] > 0)
            d = os.path.join(args.vis, "render_frames")
            os.makedirs(d, exist_ok=True)
            vis._save_png(os.path.join(d, "fused_raycast_%03d.png" % i), (rc["colors"][0][..., :3].float() * shade[..., None]).round().to(torch.uint8).cpu().numpy())
            self.pictures += 1

    def report(self):
        v = self.session.volume
        print("fused %d frames as they arrived: %d bricks of %d in a virtual grid of %s voxels, %.1f MB held, %d of %d frames tracked%s" %
              (self.session.frames, v.n_bricks, v.table.numel(), v.dims, v.memory_bytes / 1e6, sum(self.session.tracked[1:]),
               max(self.session.frames - 1, 0), ", %d ray-cast pictures written" % self.pictures if self.args.vis else ""))


def stream_loop(model, batch, args):
    """--stream: the batch through a streaming session, frame by frame, as a camera loop would (a synchronise after every push; the
    sequence `--repeat` times on the same session, the last pass is reported).  -> (preds, preds_all) as forward returns them."""
    import os
    import numpy as np
    from spann3r_amd import vis

    def image_of(i):
        img = (batch[i]["img"].permute(0, 2, 3, 1).float() + 1.0) / 2.0
        return img.swapaxes(1, 2) if img.shape[1:3] != shape else img

    n = len(batch)
    with model.stream() as s:
        for it in range(args.repeat):
            last = it == args.repeat - 1
            draw = args.vis if last else None
            s.reset()
            steps, lat, r, replays0 = [], [], None, s.replays
            fuser = StreamFuser(args) if last and args.fused and args.bricks else None
            torch.cuda.synchronize()
            start = time.time()
            for t, view in enumerate(batch):
                t0 = time.perf_counter()
                step = s.push(view)
                torch.cuda.synchronize()
                lat.append((time.perf_counter() - t0) * 1e3)
                if step is None:
                    continue
                steps.append(step)
                if draw or fuser:                                                 # final = frame t - 1, complete as of now
                    key = "pts3d" if t == 1 else "pts3d_in_other_view"
                    shape = step.final[key].shape[1:3]
                    todo = [(t - 1, step.final[key], step.final["conf"])]
                    if t == n - 1:                                                # the sequence ends here: its last frame is `latest`
                        todo.append((t, step.latest["pts3d_in_other_view"], step.latest["conf"]))
                if fuser:
                    for i, pts, conf in todo:
                        fuser.push(i, pts.float(), conf.float(), image_of(i))
                if draw:
                    if r is None:
                        d = os.path.join(draw, "render_frames")
                        os.makedirs(d, exist_ok=True)
                        camera = (vis.load_camera(args.vis_camera) if args.vis_camera else
                                  vis.fit_camera(torch.cat([step.final["pts3d"], step.latest["pts3d_in_other_view"]]).float(),
                                                 conf=torch.cat([step.final["conf"], step.latest["conf"]]).float(), conf_thresh=args.conf_thresh))
                        r = vis.PointRenderer(camera=camera, point_size=args.point_size, conf_thresh=args.conf_thresh, dynamic=args.dynamic)
                    for i, pts, conf in todo:
                        r.add(pts[0].float(), image_of(i)[0], conf[0].float())
                        vis._save_png(os.path.join(d, "frame_%03d.png" % i), r.image().cpu().numpy())
            torch.cuda.synchronize()
            end = time.time()
            print("Time: %.4f s, FPS: %.1f  (%d frames pushed one by one, pass %d%s)" %
                  (end - start, n / (end - start), n, it, (", drawing" if draw else "") + (", fusing into bricks" if fuser else "")))
            if fuser and fuser.session is not None:
                fuser.report()
        step_ms = lat[2:] or lat[1:]
        print("push latency (push + synchronise%s): median %.3f ms, p95 %.3f ms, max %.3f ms; first step %.3f ms; %d of %d pushes replayed a graph" %
              (", drawing included" if args.vis else "", float(np.median(step_ms)), float(np.percentile(step_ms, 95)), max(step_ms), lat[1],
               s.replays - replays0, n - 1))
        if args.vis:
            print("wrote %d rendered frames to %s as they arrived" % (n, os.path.join(args.vis, "render_frames")))
    return [st.final for st in steps] + [steps[-1].latest], [st.pair for st in steps]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--tiny", action="store_true", help="2-layer encoder / 10-layer decoder geometry (quick look)")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--demo_path", default=None, help="folder of images (demo.py --demo_path): decoded with PIL on the host, "
                    "then cropped / Lanczos-resized / normalised on the GPU (spann3r_amd.preprocess)")
    ap.add_argument("--kf_every", type=int, default=10)
    ap.add_argument("--save_ply", default=None, help="write the confidence-filtered cloud here (demo.py:205-212) and print the "
                    "estimated focal of the first camera (demo.py:147-151)")
    ap.add_argument("--conf_thresh", type=float, default=1e-3)
    ap.add_argument("--offline", action="store_true", help="demo.py --offline: DUSt3R pair graph + next-best-view order")
    ap.add_argument("--stream", action="store_true", help="feed the frames one at a time through model.stream() (spann3r_amd/stream.py), "
                    "synchronising after every push: prints the push latency distribution, the overall frames/s and how many pushes "
                    "replayed a graph; with --vis every frame is drawn as its prediction arrives")
    ap.add_argument("--vis", default=None, metavar="DIR", help="demo.py --vis, headless: write DIR/render_frames/frame_XXX.png (the cloud as "
                    "it grows, drawn on the device) and the pts/ imgs/ confs/ folders of vis_pred_and_imgs (spann3r_amd.vis)")
    ap.add_argument("--dynamic", action="store_true", help="demo.py --dynamic: each rendered frame shows its own points alone")
    ap.add_argument("--vis_camera", default=None, metavar="camera.json", help="render from this Open3D PinholeCameraParameters file "
                    "(e.g. one picked with the reference's find_render_cam) instead of fitting a camera to the cloud")
    ap.add_argument("--point_size", type=int, default=1)
    ap.add_argument("--vis_surface", action="store_true", help="with --vis: draw every frame as its triangle mesh (solid surfaces) "
                    "instead of one pixel per point")
    ap.add_argument("--save_glb", default=None, metavar="PATH", help="app.py's output: the confidence-masked reconstruction as one GLB, "
                    "meshed and compacted on the device (spann3r_amd.mesh)")
    ap.add_argument("--as_pointcloud", action="store_true", help="with --save_glb: app.py's as_pointcloud, points instead of a mesh")
    ap.add_argument("--fused", action="store_true", help="one welded surface instead of per-frame sheets (spann3r_amd.fusion: TSDF volume + "
                    "marching tetrahedra on the device): with --save_glb the fused mesh is what is written, with --vis a last picture "
                    "fused.png is added (and fused_raycast.png, the volume ray-cast and Lambert-shaded), with --rgbd --eval the fused prediction is scored against the fused ground truth")
    ap.add_argument("--track", action="store_true", help="with --fused: register every frame after the first to the model before it is "
                    "integrated (ray-cast the volume from the frame's pose, point-to-plane Gauss-Newton against it); prints how many "
                    "frames were tracked and the largest correction")
    ap.add_argument("--bricks", action="store_true", help="with --fused: fuse into a brick TSDF volume (fusion.BrickTSDFVolume: 8x8x8-voxel bricks "
                    "allocated where measurements land) instead of the dense one; needs --voxel_size.  With --stream --fused --bricks every "
                    "frame is posed on its own and pushed into a fusion.FusionSession as it arrives (with --vis a ray-cast picture every "
                    "--kf_every frames)")
    ap.add_argument("--direct_mesh", action="store_true", help="with --fused --bricks: mesh the bricks themselves (marching tetrahedra on the "
                    "pool, BrickTSDFVolume.extract_mesh(direct=True)) instead of densifying their bounding box first: no limit on the extent")
    ap.add_argument("--min_component", type=int, default=0, metavar="N", help="with --fused: drop the floaters -- connected components of the "
                    "fused mesh with fewer than N faces (mesh.filter_components' rule, on the device) -- from --save_glb, --vis' fused.png and "
                    "the fused --eval line; prints how many components and faces went")
    ap.add_argument("--largest_component", action="store_true", help="with --fused: keep only the connected component with the most faces")
    ap.add_argument("--simplify", type=float, default=None, metavar="CELL", help="simplify the mesh by vertex clustering on a grid of CELL, in "
                    "the units of the pointmaps (mesh.simplify, on the device): with --fused the fused surface, after --min_component; with "
                    "--save_glb alone the per-frame sheets, which it welds into one vertex set; prints the faces before and after")
    ap.add_argument("--smooth", type=int, default=0, metavar="N", help="with --fused: N rounds of Taubin's lambda|mu filter on the fused surface "
                    "(mesh.smooth, on the device: boundary vertices fixed), after --min_component and before --simplify, --save_glb, --vis' "
                    "fused.png and the fused --eval lines; --glb_normals are those of the smoothed positions")
    ap.add_argument("--fill_holes", type=int, default=0, metavar="N", help="with --fused: close every boundary loop of at most N >= 3 edges of the "
                    "fused surface (mesh.fill_holes, on the device: a fan about the mean of the loop; the rim of what was observed is a long "
                    "loop and stays open), after --min_component and before --smooth and --simplify")
    ap.add_argument("--mesh_report", action="store_true", help="with --fused: print one line on the topology of every fused surface "
                    "(mesh.topology, on the device): edges by class, Euler characteristic, closed or not; and one on its boundary loops "
                    "(mesh.boundary_loops): loops, the longest, elements on open chains, irregular vertices")
    ap.add_argument("--simplify_voxels", type=float, default=None, metavar="K", help="with --fused: --simplify with a cell of K voxels")
    ap.add_argument("--eval_samples", type=int, default=None, metavar="N", help="with --fused --rgbd --eval: a second fused line from N points "
                    "drawn by area from each fused surface with their exact face normals (evaluate.evaluate_meshes), next to the line "
                    "that scores the mesh vertices")
    ap.add_argument("--eval_exact", action="store_true", help="with --eval_samples: a third fused line, the same samples measured against "
                    "the other surface's triangles instead of its samples (evaluate.evaluate_meshes(exact=True): exact point-to-triangle "
                    "distances, the normal of the face hit)")
    ap.add_argument("--eval_cull", action="store_true", help="with --eval_samples: one more fused line, both fused surfaces first culled to "
                    "what the input views could see (mesh.cull_to_views: shadow rays against each mesh, on the device; the cull_mesh step of "
                    "NICE-SLAM-style protocols), then evaluate.evaluate_meshes; exact with --eval_exact, over a tree with --eval_bvh")
    ap.add_argument("--eval_depth", action="store_true", help="with --fused --rgbd --eval: one more fused line, the fused prediction's depth "
                    "maps from the ground-truth cameras (mesh.render_depth_maps: rays against the mesh, on the device) scored against the "
                    "RGB-D depth in image space: abs-rel, RMSE, delta < 1.25 and coverage (evaluate.evaluate_depth)")
    ap.add_argument("--eval_bvh", action="store_true", help="with --eval_exact or --eval_depth: answer them over a bounding-volume hierarchy "
                    "of the faces (mesh.TriangleBVH) instead of the uniform grid: the same numbers, at a cost that does not grow with the "
                    "distance between prediction and ground truth")
    ap.add_argument("--glb_normals", action="store_true", help="with --save_glb: write area-weighted vertex normals (mesh.vertex_normals, on "
                    "the device) as the NORMAL attribute of the fused or per-frame mesh, so that viewers light it")
    ap.add_argument("--extent", type=float, nargs=6, default=None, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"), help="with --stream --fused "
                    "--bricks: the box the session may fuse in (default: a cube of +-4 units around the first camera)")
    ap.add_argument("--voxel_size", type=float, default=None, help="with --fused: voxel edge in the units of the pointmaps (default: the "
                    "longest side of the confident points' box takes 256 voxels)")
    ap.add_argument("--trunc_voxels", type=float, default=3.0, help="with --fused: truncation distance in voxels")
    ap.add_argument("--clean", type=float, default=None, metavar="TOL", help="clean the confidences across the frames before anything reads "
                    "them (spann3r_amd.multiview.clean_sequence, on the device: DUSt3R's clean_pointcloud rule): a pixel that floats in "
                    "front of what a more confident frame measured, by more than the relative depth tolerance TOL, gets confidence 0 and "
                    "so leaves --save_ply, --save_glb, --vis, --fused and --eval; prints the pixels clipped per frame and in total")
    ap.add_argument("--clean_order", default="sequence", choices=["parallel", "sequence"], help="with --clean: judge every frame against "
                    "the original confidences (parallel, one launch) or frame by frame against the already cleaned ones (sequence)")
    ap.add_argument("--min_agree", type=int, default=0, metavar="K", help="with --clean: also drop every pixel that fewer than K other frames "
                    "agree with or that any frame looks through (multiview.support_mask); 0: off")
    ap.add_argument("--global_align", action="store_true", help="DUSt3R's global alignment (spann3r_amd.align.GlobalAligner, on the device): "
                    "the DUSt3R pair graph of the frames is aligned into one set of poses, focals and depth maps, and the aligned pointmaps "
                    "(in the first camera's frame), its confidences, poses and focals replace forward's prediction for --save_ply, --save_glb, "
                    "--vis, --fused and --clean; prints edges, initial loss, final loss, iterations")
    ap.add_argument("--align_iters", type=int, default=300, metavar="N", help="with --global_align: iterations of the optimiser")
    ap.add_argument("--align_graph", default="complete", metavar="GRAPH", help="with --global_align: the pair graph, make_pairs' scene_graph "
                    "(complete, swin-K, oneref-K, ...)")
    ap.add_argument("--rgbd", default=None, metavar="DIR", help="folder of *.npz frames (rgb uint8 [H,W,3], depth uint16 or float32 [H,W], "
                    "K [3,3], pose [4,4] cam2world; tools/make_rgbd_folder.py writes one): views with ground truth built on the GPU "
                    "(spann3r_amd.views.build_views) instead of synthetic frames")
    ap.add_argument("--eval", action="store_true", help="with --rgbd: eval.py's alignment and reconstruction metrics for the sequence "
                    "(spann3r_amd.evaluate.evaluate_sequence)")
    ap.add_argument("--depth_div", type=float, default=1000.0, help="with --rgbd: raw depth units per metre")
    ap.add_argument("--raw_invalid", type=float, default=65535, help="with --rgbd: raw value that means no measurement")
    ap.add_argument("--max_depth", type=float, default=10.0)
    ap.add_argument("--min_depth", type=float, default=1e-3)
    args = ap.parse_args()
    if args.bricks and not (args.fused and args.voxel_size):
        ap.error("--bricks needs --fused and --voxel_size")
    if args.direct_mesh and not args.bricks:
        ap.error("--direct_mesh needs --bricks")
    if (args.min_component or args.largest_component) and not args.fused:
        ap.error("--min_component / --largest_component need --fused")
    if args.min_component < 0:
        ap.error("--min_component must be >= 0")
    if (args.smooth or args.mesh_report or args.fill_holes) and not args.fused:
        ap.error("--smooth / --fill_holes / --mesh_report need --fused (a fused surface)")
    if args.fill_holes != 0 and args.fill_holes < 3:
        ap.error("--fill_holes must be 0 or >= 3 (the shortest loop)")
    if args.smooth < 0:
        ap.error("--smooth must be >= 0")
    if args.simplify_voxels is not None and not args.fused:
        ap.error("--simplify_voxels needs --fused (a voxel size)")
    if args.simplify is not None and not (args.fused or args.save_glb):
        ap.error("--simplify needs --fused or --save_glb (a mesh to simplify)")
    if args.simplify is not None and args.simplify_voxels is not None:
        ap.error("--simplify and --simplify_voxels exclude each other")
    if args.eval_samples is not None and not (args.fused and args.rgbd and args.eval):
        ap.error("--eval_samples needs --fused --rgbd --eval (two fused surfaces to sample)")
    if args.eval_samples is not None and args.eval_samples <= 0:
        ap.error("--eval_samples must be positive")
    if args.eval_exact and args.eval_samples is None:
        ap.error("--eval_exact needs --eval_samples (the samples it measures against the other surface's triangles)")
    if args.eval_cull and args.eval_samples is None:
        ap.error("--eval_cull needs --eval_samples (the samples drawn from the culled surfaces)")
    if args.eval_bvh and not (args.eval_exact or args.eval_depth):
        ap.error("--eval_bvh needs --eval_exact or --eval_depth (the evaluations that query the faces of a mesh)")
    if args.eval_depth and not (args.fused and args.rgbd and args.eval):
        ap.error("--eval_depth needs --fused --rgbd --eval (a fused surface and ground-truth depth maps to score it against)")
    if args.min_agree < 0 or (args.min_agree and args.clean is None):
        ap.error("--min_agree must be >= 0 and needs --clean (its depth tolerance)")
    if args.clean is not None and not 0.0 <= args.clean < 1.0:
        ap.error("--clean must lie in [0, 1)")
    if args.glb_normals and not args.save_glb:
        ap.error("--glb_normals needs --save_glb (a file to write them to)")
    if args.global_align and (args.stream or args.offline or args.align_iters < 1):
        ap.error("--global_align aligns forward's frames: not with --stream or --offline, and --align_iters must be >= 1")
    if args.glb_normals and args.as_pointcloud:
        ap.error("--glb_normals needs a mesh: a point cloud (--as_pointcloud) has no faces to take normals from")
    for name in ("simplify", "simplify_voxels"):
        if getattr(args, name) is not None and not (getattr(args, name) > 0 and math.isfinite(getattr(args, name))):
            ap.error("--%s must be positive and finite" % name)
    cfg = TINY if args.tiny else FULL
    device = "cuda"
    model = Spann3R(dus3r_name=None, cfg=cfg, init_weights=False).to(device)      # demo.py:81-82
    model.load_state_dict(synth_state_dict(0, cfg))                               # demo.py:84 (no checkpoint ships)
    model.eval().set_precision(args.precision)
    if args.demo_path:                                                            # demo.py:86-92 (Demo dataset, full_video)
        import os
        import numpy as np
        from PIL import Image
        from spann3r_amd.preprocess import frames_from_images
        names = sorted(n for n in os.listdir(args.demo_path) if n.lower().endswith((".jpg", ".jpeg", ".png")))
        batch = frames_from_images((np.asarray(Image.open(os.path.join(args.demo_path, n)).convert("RGB")) for n in names),
                                   resolution=args.size, device=device, kf_every=args.kf_every)
    elif args.rgbd:                                                               # eval.py:79-87 (a data set + DataLoader(batch_size=1))
        import os
        import numpy as np
        from spann3r_amd.views import build_views
        names = sorted(n for n in os.listdir(args.rgbd) if n.endswith(".npz"))[::args.kf_every]
        data = [np.load(os.path.join(args.rgbd, n)) for n in names]
        cols = [[d[k] for d in data] for k in ("rgb", "depth", "K", "pose")]
        kw = dict(resolution=args.size, device=device, depth_div=args.depth_div, raw_invalid=args.raw_invalid, min_depth=args.min_depth,
                  max_depth=args.max_depth, labels=[os.path.join(os.path.basename(os.path.normpath(args.rgbd)), n) for n in names])
        build_views(*cols, **kw)                                                  # warm-up: resampling tables, first launches
        torch.cuda.synchronize()
        start = time.time()
        batch = build_views(*cols, **kw)
        torch.cuda.synchronize()
        end = time.time()
        print("build_views: %d views of %dx%d -> %s in %.4f s, %.0f views/s, %.1f %% of the pixels valid" %
              (len(batch), data[0]["rgb"].shape[1], data[0]["rgb"].shape[0], tuple(batch[0]["img"].shape[2:]), end - start,
               len(batch) / (end - start), 100 * float(torch.cat([v["valid_mask"] for v in batch]).float().mean())))
    else:
        batch = synth_frames(args.frames, args.size, args.size)
    if args.eval and not args.rgbd:
        ap.error("--eval needs --rgbd (views with ground truth)")
    for view in batch if not (args.demo_path or args.rgbd) else []:                                                            # demo.py:94-95
        view["img"] = view["img"].to(device, non_blocking=True)
        view["true_shape"] = torch.tensor(view["img"].shape[2:]).unsqueeze(0)     # demo.py:109 (stays on the CPU)
    if args.offline:                                                              # demo.py:98-121
        from spann3r_amd.runner import pair_graph
        torch.cuda.synchronize()
        start = time.time()
        output = pair_graph(model.dust3r, batch)          # = make_pairs(complete, symmetrize) + inference(batch_size=2)
        preds, preds_all, idx_used = model.offline_reconstruction(batch, output)
        torch.cuda.synchronize()
        end = time.time()
        print("Time: %.4f s, FPS: %.1f  (offline, order %s)" % (end - start, len(batch) / (end - start), idx_used))
        return
    if args.stream:
        preds, preds_all = stream_loop(model, batch, args)
    for it in range(0 if args.stream else args.repeat):
        torch.cuda.synchronize()
        start = time.time()
        preds, preds_all = model.forward(batch)                                   # demo.py:125
        torch.cuda.synchronize()
        end = time.time()
        print("Time: %.4f s, FPS: %.1f  (%d frames, call %d: %s)" %
              (end - start, len(batch) / (end - start), len(batch), it,
               ["eager warm-up", "hipGraph capture", "hipGraph replay"][min(it, 2)]))
    aligned = None
    if args.global_align:                                                         # once, in front of every consumer of the prediction
        from spann3r_amd.align import GlobalAligner
        from spann3r_amd.runner import pair_graph
        with torch.no_grad():
            graph = pair_graph(model.dust3r, batch, scene_graph=args.align_graph)
        torch.cuda.synchronize()
        start = time.time()
        scene = GlobalAligner(graph)
        final = scene.compute_global_alignment(init="mst", niter=args.align_iters)
        torch.cuda.synchronize()
        print("global alignment: %d edges, initial loss %.6g, final loss %.6g, %d iterations (%.3f s)" %
              (scene.n_edges, scene.losses[0], final, len(scene.losses), time.time() - start))
        with torch.no_grad():                                                     # everything in the first camera's frame, as forward gives it
            poses = scene.get_im_poses().double().cpu()
            to_first = torch.linalg.inv(poses[0])
            poses = (to_first @ poses).numpy()
            R0, t0 = to_first[:3, :3].float().to(device), to_first[:3, 3].float().to(device)
            aligned = dict(poses=poses, K=scene.get_intrinsics().double().cpu().numpy())
            preds = [{("pts3d" if j == 0 else "pts3d_in_other_view"): (p @ R0.T + t0)[None].to(preds[j]["conf"].dtype),
                      "conf": c[None].to(preds[j]["conf"].dtype)} for j, (p, c) in enumerate(zip(scene.get_pts3d(), scene.im_conf))]
    if args.clean is not None:                                                    # once, in front of every consumer of the confidences
        import numpy as np
        from spann3r_amd import multiview
        kw = dict(tol=args.clean, order=args.clean_order)
        try:
            if aligned is not None:                                               # the aligned cameras: every image's own intrinsics
                from spann3r_amd import mesh as M
                pts_c, _, conf_all = M.sequence_tensors(preds, batch)
                conf_c = multiview.clean_confidence(pts_c, conf_all, aligned["K"], aligned["poses"], **kw)
                info = dict(poses=aligned["poses"], K=aligned["K"],
                            cleaned=(conf_c.view(torch.int32) != conf_all.contiguous().view(torch.int32)).flatten(1).sum(1).cpu().tolist())
            else:
                pts_c, _, conf_c, info = multiview.clean_sequence(preds, batch, **kw)
        except RuntimeError as e:
            if "degenerate pointmaps" not in str(e):
                raise
            _, H, W, _ = preds[0]["pts3d"].shape
            print("%s: cleaning through nominal cameras (focal %d, identity poses)" % (e, max(H, W)))
            pts_c, _, conf_c, info = multiview.clean_sequence(preds, batch, focal=float(max(H, W)), poses=np.stack([np.eye(4)] * len(preds)), **kw)
        print("cleaned confidences (tol %g, %s order): pixels clipped per frame %s, %d of %d in total" %
              (args.clean, args.clean_order, info["cleaned"], sum(info["cleaned"]), conf_c.numel()))
        if args.min_agree:
            _, H, W, _ = pts_c.shape
            K = info["K"] if "K" in info else np.array([[info["focal"], 0, W / 2], [0, info["focal"], H / 2], [0, 0, 1]], np.float64)
            keep = multiview.support_mask(multiview.view_consistency(pts_c, K, info["poses"], conf=conf_c, tol=args.clean), args.min_agree)
            print("support: %d of %d pixels have at least %d agreeing frames and none looking through them" %
                  (int(keep.sum()), keep.numel(), args.min_agree))
            conf_c = torch.where(keep, conf_c, torch.zeros_like(conf_c))
        preds = [dict(p, conf=conf_c[j:j + 1].to(p["conf"].dtype)) for j, p in enumerate(preds)]
    fuse_kw = dict(voxel_size=args.voxel_size, trunc_voxels=args.trunc_voxels, min_component_faces=args.min_component,
                   keep_largest=1 if args.largest_component else None, smooth_iters=args.smooth, fill_holes=args.fill_holes)
    if args.simplify is not None:
        fuse_kw["simplify_cell"] = args.simplify
    elif args.simplify_voxels is not None and args.voxel_size:
        fuse_kw["simplify_cell"] = args.simplify_voxels * args.voxel_size

    def report_simplify(what, fm):
        s = fm.get("simplify")
        if s is not None:
            print("%s: simplified on a grid of %g: %d faces -> %d (%d collapsed, %d duplicate, %d invalid), %d clusters -> %d vertices" %
                  (what, s["cell"], s["faces_in"], 0 if fm["faces"] is None else fm["faces"].shape[0], s["faces_collapsed"], s["faces_duplicate"],
                   s["faces_invalid"], s["clusters"], fm["vertices"].shape[0]))

    def report_topology(what, fm):
        s = fm.get("fill")
        if s is not None:
            print("%s: %d of %d boundary loops of at most %d edges filled: %d vertices and %d faces added (%d boundary edges on open chains)" %
                  (what, s["filled"], s["loops"], s["max_edges"], s["vertices_added"], s["faces_added"], s["open"]))
        s = fm.get("smooth")
        if s is not None:
            print("%s: smoothed by %d rounds of lambda %g | mu %g, %d boundary vertices fixed" %
                  (what, s["iterations"], s["lam"], s["mu"], s["fixed_vertices"]))
        if args.mesh_report and fm.get("faces") is not None:
            from spann3r_amd.mesh import boundary_loops, topology
            topo = topology(fm)
            r = topo.report
            print("%s: %d edges (%d boundary, %d interior, %d inconsistent, %d non-manifold), %d usable faces (%d unusable), %d vertices "
                  "referenced, Euler characteristic %d, %s" %
                  (what, r["edges"], r["boundary"], r["interior"], r["inconsistent"], r["nonmanifold"], r["faces_usable"], r["faces_unusable"],
                   r["vertices_referenced"], r["euler"], "closed" if r["closed"] else "open"))
            r = boundary_loops(fm, topo).report
            print("%s: %d boundary edges in %d loops (the longest %d), %d on open chains, %d irregular boundary vertices" %
                  (what, r["boundary"], r["loops"], r["longest"], r["open"], r["irregular_vertices"]))

    def report_components(what, fm):
        c = fm.get("components")
        if c is not None:
            print("%s: %d connected components, %d kept; %d components and %d faces removed" %
                  (what, c["total"], c["kept"], c["total"] - c["kept"], c["faces_removed"]))

    def fused_prediction(**kw):
        """fusion.fuse_sequence of this run (demo.py's focal and poses) -> (mesh, volume); pointmaps without geometry (no checkpoint
        ships) are fused through nominal cameras instead -- focal = the longer image side, identity poses -- and that is said.
        With --track the frames are registered to the model first and the corrections are reported."""
        from spann3r_amd import fusion
        import numpy as np
        kw = dict(conf_thresh=args.conf_thresh, return_volume=True, track=args.track, return_poses=args.track, bricks=args.bricks,
                  direct_mesh=args.direct_mesh, **fuse_kw, **kw)
        try:
            if aligned is not None:                                               # the aligned cameras, not estimates from the pointmaps
                from spann3r_amd import mesh as M
                pts_all, images_all, conf_all = M.sequence_tensors(preds, batch)
                fm, vol = fusion.fuse_pointmaps(pts_all, aligned["K"], aligned["poses"], (conf_all - 1) / conf_all > args.conf_thresh, images_all,
                                                **{k: v for k, v in kw.items() if k != "conf_thresh"})
            else:
                fm, vol = fusion.fuse_sequence(preds, batch, **kw)
        except RuntimeError as e:
            if "degenerate pointmaps" not in str(e):
                raise
            _, H, W, _ = preds[0]["pts3d"].shape
            print("%s: fusing through nominal cameras (focal %d, identity poses)" % (e, max(H, W)))
            fm, vol = fusion.fuse_sequence(preds, batch, focal=float(max(H, W)), poses=np.stack([np.eye(4)] * len(preds)), **kw)
        if args.simplify_voxels is not None and "simplify_cell" not in kw:      # no --voxel_size: the cell follows the volume's own voxel
            fm = dict(fm, **vol.extract_mesh(scale=kw.get("scale", 1.0), transform=kw.get("transform"), min_component_faces=args.min_component,
                                             keep_largest=kw["keep_largest"], simplify_cell=args.simplify_voxels * vol.voxel_size,
                                             smooth_iters=args.smooth, fill_holes=args.fill_holes))
        if args.track:
            T = fm["corrections"][1:]
            ang = [math.degrees(math.acos(min(max((np.trace(t[:3, :3]) - 1) * 0.5, -1.0), 1.0))) for t in T]
            print("%d frames tracked of %d; largest correction %.3f degrees, %.3f voxels" %
                  (sum(fm["tracked"][1:]), len(T), max(ang, default=0.0), max((np.linalg.norm(t[:3, 3]) for t in T), default=0.0) / vol.voxel_size))
        report_components("fused surface", fm)
        report_topology("fused surface", fm)
        report_simplify("fused surface", fm)
        return fm, vol

    if args.eval:                                                                 # eval.py:128-221
        from spann3r_amd.evaluate import evaluate_sequence
        r = evaluate_sequence(batch, preds, preds_all, threshold=0.1)
        print("Idx: %s, Acc: %s, Comp: %s, NC1: %s, NC2: %s - Acc_med: %s, Compc_med: %s, NC1c_med: %s, NC2c_med: %s  (%d points)" %
              (batch[-1]["label"].rsplit("/", 1)[0], r["acc"], r["comp"], r["nc1"], r["nc2"], r["acc_med"], r["comp_med"], r["nc1_med"],
               r["nc2_med"], len(r["pred_cloud"])))
        if args.fused:                                                            # the surfaces instead of the per-pixel clouds
            from spann3r_amd import fusion
            from spann3r_amd.evaluate import align_to_ground_truth, evaluate_reconstruction
            a = align_to_ground_truth(batch, preds, preds_all)
            gt_mesh = fusion.fuse_views(batch, **fuse_kw)
            pred_mesh = fusion.fuse_pointmaps(a["pts_all"], torch.cat([v["camera_intrinsics"] for v in batch]),
                                              torch.cat([v["camera_pose"] for v in batch]), a["masks_all"], a["images_all"], **fuse_kw)
            report_components("fused ground truth", gt_mesh)
            report_components("fused prediction", pred_mesh)
            report_topology("fused ground truth", gt_mesh)
            report_topology("fused prediction", pred_mesh)
            rf = evaluate_reconstruction(pred_mesh["vertices"], gt_mesh["vertices"], threshold=0.1)
            print("Fused: Acc: %s, Comp: %s, NC1: %s, NC2: %s  (prediction %d vertices / %d faces, ground truth %d vertices / %d faces)" %
                  (rf["acc"], rf["comp"], rf["nc1"], rf["nc2"], pred_mesh["vertices"].shape[0], pred_mesh["faces"].shape[0],
                   gt_mesh["vertices"].shape[0], gt_mesh["faces"].shape[0]))
            if args.eval_samples is not None:
                from spann3r_amd.evaluate import evaluate_meshes
                rs = evaluate_meshes(pred_mesh, gt_mesh, n_samples=args.eval_samples, threshold=0.1)
                print("Fused (area-sampled, %d): Acc: %s, Comp: %s, NC1: %s, NC2: %s  (prediction area %.6g, ground truth area %.6g)" %
                      (rs["samples"], rs["acc"], rs["comp"], rs["nc1"], rs["nc2"], rs["pred_area"], rs["gt_area"]))
                if args.eval_exact:
                    rx = evaluate_meshes(pred_mesh, gt_mesh, n_samples=args.eval_samples, threshold=0.1, exact=True,
                                         accel="bvh" if args.eval_bvh else None)
                    print("Fused (exact, %d): Acc: %s, Comp: %s, NC1: %s, NC2: %s" % (rx["samples"], rx["acc"], rx["comp"], rx["nc1"], rx["nc2"]))
                if args.eval_cull:                                                # both surfaces culled to what the input views observe
                    h, w = batch[0]["depthmap"].shape[-2:]
                    cams = dict(intrinsics=torch.cat([v["camera_intrinsics"] for v in batch]), cam2world=torch.cat([v["camera_pose"] for v in batch]),
                                size=(h, w))
                    rc = evaluate_meshes(pred_mesh, gt_mesh, n_samples=args.eval_samples, threshold=0.1, exact=args.eval_exact,
                                         accel="bvh" if args.eval_exact and args.eval_bvh else None, cull_views=cams)
                    print("Fused (culled to %d views, %d): Acc: %s, Comp: %s, NC1: %s, NC2: %s  (faces kept: prediction %d of %d, ground truth %d of %d)" %
                          (len(batch), rc["samples"], rc["acc"], rc["comp"], rc["nc1"], rc["nc2"], rc["pred_faces_kept"], pred_mesh["faces"].shape[0],
                           rc["gt_faces_kept"], gt_mesh["faces"].shape[0]))
            if args.eval_depth:
                from spann3r_amd.evaluate import evaluate_depth
                rd = evaluate_depth(pred_mesh, batch, bvh=True if args.eval_bvh else None)
                print("Fused (depth, %d views): AbsRel: %s, RMSE: %s, Delta1: %s, Coverage: %s  (%d pixels compared)" %
                      (rd["views"], rd["abs_rel"], rd["rmse"], rd["delta1"], rd["coverage"], rd["pixels"]))
    if args.save_ply:
        from spann3r_amd.postprocess import (estimate_focal_knowing_depth, confident_points, write_ply, estimate_poses,
                                             transforms_json, save_transforms)
        _, H, W, _ = preds[0]["pts3d"].shape
        focal = estimate_focal_knowing_depth(preds[0]["pts3d"], torch.tensor((W / 2, H / 2)), focal_mode="weiszfeld")
        print("Estimated focal of first camera: %.3f (%dx%d)" % (focal.item(), W, H))
        pts_all = torch.cat([p["pts3d" if j == 0 else "pts3d_in_other_view"] for j, p in enumerate(preds)])
        conf_all = torch.cat([p["conf"] for p in preds])
        images_all = (torch.cat([v["img"] for v in batch]).permute(0, 2, 3, 1) + 1.0) / 2.0
        if images_all.shape[1:3] != pts_all.shape[1:3]:
            images_all = images_all.swapaxes(1, 2)                                # portrait frames were rectified to landscape
        points, colours = confident_points(pts_all, conf_all, args.conf_thresh, images_all)
        import os
        os.makedirs(os.path.dirname(os.path.abspath(args.save_ply)), exist_ok=True)
        write_ply(args.save_ply, points, colours)
        print("wrote %d of %d points to %s" % (len(points), conf_all.numel(), args.save_ply))
        if focal.item() > 1e-3:                                                 # (seeded random weights give no geometry at all)
            poses_all, inliers = estimate_poses(pts_all, focal, (W / 2, H / 2))     # demo.py:170-186 (PnP-RANSAC per frame)
            tj = os.path.join(os.path.dirname(os.path.abspath(args.save_ply)), "transforms.json")
            save_transforms(tj, transforms_json(H, W, focal, list(poses_all), os.path.basename(args.save_ply)))
            print("wrote %d camera poses to %s (inlier fractions %.2f..%.2f)" % (len(poses_all), tj, inliers.min(), inliers.max()))
        else:
            print("degenerate pointmaps (no checkpoint loaded): poses / transforms.json skipped")
    if args.vis and not args.stream:                                              # demo.py:221-225 (--stream drew as it went)
        from spann3r_amd import vis
        pts_all = torch.cat([p["pts3d" if j == 0 else "pts3d_in_other_view"] for j, p in enumerate(preds)]).float()
        conf_all = torch.cat([p["conf"] for p in preds]).float()
        conf_sig_all = (conf_all - 1) / conf_all                                  # demo.py:213
        images_all = (torch.cat([v["img"] for v in batch]).permute(0, 2, 3, 1).float() + 1.0) / 2.0
        if images_all.shape[1:3] != pts_all.shape[1:3]:
            images_all = images_all.swapaxes(1, 2)
        camera = (vis.load_camera(args.vis_camera) if args.vis_camera else
                  vis.fit_camera(pts_all, conf=conf_all, conf_thresh=args.conf_thresh))      # stands in for find_render_cam
        vis.render_frames(pts_all, images_all, camera, args.vis, conf_all=conf_all, conf_thresh=args.conf_thresh, dynamic=args.dynamic,
                          point_size=args.point_size, surface=args.vis_surface)
        vis.vis_pred_and_imgs(pts_all, args.vis, images_all=images_all, conf_all=conf_sig_all)
        if args.fused:
            import os
            fm, vol = fused_prediction()
            r = vis.PointRenderer(camera=camera)
            r.add_triangles(fm["vertices"], fm["faces"], fm["colors"])
            vis._save_png(os.path.join(args.vis, "render_frames", "fused.png"), r.image().cpu().numpy())
            print("wrote the fused surface (%d vertices, %d faces) as render_frames/fused.png" % (fm["vertices"].shape[0], fm["faces"].shape[0]))
            import numpy as np
            c2w = np.linalg.inv(camera.extrinsic)                                 # the same volume with no meshing: ray-cast, Lambert-shaded
            rc = vol.raycast(camera.intrinsic, c2w, (camera.height, camera.width))
            view = rc["vertices"][0] - torch.from_numpy(c2w[:3, 3]).to(rc["vertices"])
            view = view / view.norm(dim=-1, keepdim=True).clamp_min(1e-30)
            shade = (-(rc["normals"][0] * view).sum(-1)).clamp_min(0.0) * (rc["depth"][0] > 0)
            colour = rc["colors"][0][..., :3].float() if "colors" in rc else torch.full_like(rc["vertices"][0], 255.0)
            vis._save_png(os.path.join(args.vis, "render_frames", "fused_raycast.png"), (colour * shade[..., None]).round().to(torch.uint8).cpu().numpy())
            print("wrote the ray-cast volume (%d of %d pixels hit) as render_frames/fused_raycast.png" % (int((rc["depth"] > 0).sum()), rc["depth"].numel()))
        print("wrote %d rendered frames (%dx%d%s) and pts/ imgs/ confs/ to %s" %
              (len(pts_all), camera.width, camera.height, (", dynamic" if args.dynamic else "") + (", surface" if args.vis_surface else ""), args.vis))
    if args.save_glb:                                                             # app.py:132-171
        import os
        from spann3r_amd import mesh
        os.makedirs(os.path.dirname(os.path.abspath(args.save_glb)), exist_ok=True)
        if args.fused:
            fm, _ = fused_prediction(scale=mesh.SCALE, transform=mesh.TRANSFORM)      # app.py's x10 and axis flip, as export_glb
            if fm["faces"].shape[0] == 0 and fm.get("components", {}).get("total", 0) > 0:
                raise RuntimeError("--fused: --min_component %d%s removed every one of the %d components of the surface" %
                                   (args.min_component, " / --largest_component" if args.largest_component else "", fm["components"]["total"]))
            if fm["faces"].shape[0] == 0:
                raise RuntimeError("--fused: the volume holds no surface (nothing passes conf_thresh %g with weight >= 1)" % args.conf_thresh)
            size = mesh.write_glb(args.save_glb, fm["vertices"], fm["colors"], fm["faces"], bounds=fm["bounds"],
                                  normals=mesh.vertex_normals(fm) if args.glb_normals else None)
            info = dict(vertices=fm["vertices"].shape[0], faces=fm["faces"].shape[0], bytes=size)
        elif args.simplify is not None:                                           # the sheets welded: one vertex per cell of all frames
            scene = mesh.scene_mesh(*mesh.sequence_tensors(preds, batch), args.conf_thresh, args.as_pointcloud)
            scene = mesh.simplify(scene, args.simplify * mesh.SCALE)                 # (the sheets are already in the GLB's x10 units)
            report_simplify("per-frame sheets", scene)
            if scene["vertices"].shape[0] == 0:
                raise RuntimeError("--simplify %g left nothing of the sheets to write" % args.simplify)
            size = mesh.write_glb(args.save_glb, scene["vertices"], scene["colors"], scene["faces"], bounds=scene["bounds"],
                                  normals=mesh.vertex_normals(scene) if args.glb_normals else None)
            info = dict(vertices=scene["vertices"].shape[0], faces=0 if scene["faces"] is None else scene["faces"].shape[0], bytes=size)
        elif args.glb_normals:                                                    # export_glb's mesh with its vertex normals
            scene = mesh.scene_mesh(*mesh.sequence_tensors(preds, batch), args.conf_thresh)
            if scene["faces"].shape[0] == 0:
                raise RuntimeError("--glb_normals: nothing passes conf_thresh %g: no face to write" % args.conf_thresh)
            size = mesh.write_glb(args.save_glb, scene["vertices"], scene["colors"], scene["faces"], bounds=scene["bounds"],
                                  normals=mesh.vertex_normals(scene))
            info = dict(vertices=scene["vertices"].shape[0], faces=scene["faces"].shape[0], bytes=size)
        else:
            info = mesh.export_glb(args.save_glb, preds, batch, conf_thresh=args.conf_thresh, as_pointcloud=args.as_pointcloud)
        print("wrote %d vertices, %d faces (%d bytes) to %s" % (info["vertices"], info["faces"], info["bytes"], args.save_glb))
    pts = preds[-1]["pts3d_in_other_view"]
    print("last frame: pts3d_in_other_view", tuple(pts.shape), "conf mean %.3f" % float(preds[-1]["conf"].mean()))


if __name__ == "__main__":
    main()
