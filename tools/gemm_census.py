"""The GEMM launch census: every distinct auto-tile (tile < 0) launch the model issues, as tests/golden/gemm_plan_table.jsonl keeps it.

  with gemm_census.capture() as seen: ... run the model ...      seen = [{"descs": [..], "lean": 0 | 1, "tiles": [..]}, ..] (distinct)
  python tools/gemm_census.py --diff bf16_224 fp32_224             runs those configurations and lists launches the table lacks,
                                                                   each next to the table row it differs least from
  python tools/gemm_census.py --write bf16_224 ...                  adds them to the table; a launch that is already a row only gets
                                                                   the configuration's tag merged into the row's `from` list

A descriptor is normalised as the table does: pointers as set / not set, zero fields left out (alpha and batch always kept), strides,
per-problem byte offsets, ln_eps, sm_thresh, tile and trace dropped -- no planning rule reads them.

Which `from` tags this tool produces.  CONFIGS holds the inference configurations with the number of frames the table was taken at
(the whole-sequence encoder's row count and the memory bank's extents depend on it): bf16_224 and fp32_224 are checked on the device
by tests/test_gemm_census_gpu.py::test_census_is_current; the frame counts of the other entries are read off the table's shapes and
not verified.  Rows recorded with the lean instances off (`lean`: 0) come from the same configurations in a process started with
SP3_LEAN_GEMM=0, the `+levels0` tags from one started with SP3_HEAD_LEVELS=0 (both variables are read once per process; the tag and
the `lean` field follow them).  The training tags (train_fp32, train_bf16: 180 rows) have no producer here: they were taken from
spann3r_amd.train's step and this tool does not drive it.
"""
import ctypes as C
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
TABLE = os.path.join(REPO, "tests", "golden", "gemm_plan_table.jsonl")
DROPPED = {"strideA", "strideW", "strideC", "ln_eps", "sm_thresh", "tile", "trace"}
# name -> (precision, height, width, batch, frames)
CONFIGS = {"bf16_224": ("bf16", 224, 224, 1, 10), "fp32_224": ("fp32", 224, 224, 1, 4), "f16x3_224": ("f16x3", 224, 224, 1, 4),
           "bf16_512": ("bf16", 512, 512, 1, 8), "f16x3_512": ("f16x3", 512, 512, 1, 4), "bf16_224_b4": ("bf16", 224, 224, 4, 4)}


def normalise(d):
    from spann3r_amd import lib as L
    out = {}
    for name, ctype in L.GemmDesc._fields_:
        if name in DROPPED or name.startswith("sb_"):
            continue
        v = getattr(d, name)
        if ctype is C.c_void_p:
            if v:
                out[name] = 1
        elif v or name in ("alpha", "batch"):
            out[name] = v
    return out


def key(row):
    return json.dumps([row["descs"], row["lean"], row["tiles"]], sort_keys=True)


class capture:
    """records the distinct auto-tile launches issued inside (ops._gemm_launch and the grouped path of ops.level)"""

    def __enter__(self):
        from spann3r_amd import lib as L, ops
        self.ops, self.seen, self._keys = ops, [], set()
        self._launch, self._send = ops._gemm_launch, ops.level._send
        lean = int(ops.LEAN)

        def note(ds):
            if any(d.tile >= 0 for d in ds):
                return
            if len(ds) == 1:
                tiles = [int(L.load().sp3_gemm_plan(C.byref(ds[0])))]
            else:
                arr = (C.POINTER(L.GemmDesc) * len(ds))(*[C.pointer(d) for d in ds])
                t = (C.c_int * len(ds))()
                tiles = list(t) if L.load().sp3_gemm_plan_n(arr, len(ds), t) == 0 else [-1] * len(ds)
            row = {"descs": [normalise(d) for d in ds], "lean": lean, "tiles": tiles}
            if key(row) not in self._keys:
                self._keys.add(key(row))
                self.seen.append(row)

        def launch(d, what, name):
            if ops._held is None:
                note([d])
            return self._launch(d, what, name)

        def send(group, is_conv):
            if len(group) > 1:
                note([g[0] for g in group])
            return self._send(group, is_conv)          # (one descriptor: goes through _gemm_launch)
        ops._gemm_launch, ops.level._send = launch, staticmethod(send)
        return self.seen

    def __exit__(self, *exc):
        self.ops._gemm_launch, self.ops.level._send = self._launch, staticmethod(self._send)
        return False


def load_table():
    return [json.loads(line) for line in open(TABLE)]


def tag(name):
    from spann3r_amd import ops
    return name + ("" if ops.HEAD_LEVELS else "+levels0")


def run_config(model, name, frames=None):
    """the launches of configuration `name` (its own number of frames unless given) on a FULL model"""
    from spann3r_amd.weights import synth_frames
    precision, h, w, batch, nframes = CONFIGS[name]
    frames = frames or nframes
    model.set_precision(precision)
    with capture() as seen:
        model([{"img": f["img"].to("cuda")} for f in synth_frames(frames, h, w, batch=batch)])
    return seen


def missing(seen, table=None):
    have = {key(r) for r in (load_table() if table is None else table)}
    return [r for r in seen if key(r) not in have]


def nearest(row, table):
    """(line, fields that differ) of the table row of as many descriptors that differs least from `row`: tells a stale table (a new
    shape) from a capture taken differently (frames, product mode, lean)"""
    best = None
    for i, t in enumerate(table):
        if len(t["descs"]) != len(row["descs"]):
            continue
        diff = {}
        for j, (a, b) in enumerate(zip(row["descs"], t["descs"])):
            for k in set(a) | set(b):
                if a.get(k, 0) != b.get(k, 0):
                    diff["%d.%s" % (j, k)] = (a.get(k, 0), b.get(k, 0))
        for k in ("lean", "tiles"):
            if row[k] != t[k]:
                diff[k] = (row[k], t[k])
        if best is None or len(diff) < len(best[1]):
            best = (i + 1, diff)
    return best


def describe_missing(new, table, limit=8):
    return "\n".join("%s\n    nearest: line %d, differs in %r" % ((json.dumps(r, sort_keys=True),) + nearest(r, table)) for r in new[:limit])


def main(argv):
    import torch  # noqa: F401
    from spann3r_amd import Spann3R, FULL
    from spann3r_amd.weights import synth_state_dict
    mode, names = argv[0], argv[1:]
    m = Spann3R(dus3r_name=None, cfg=FULL, init_weights=False)
    m.load_state_dict(synth_state_dict(0, FULL), strict=True)
    m = m.to("cuda").eval()
    table = load_table()
    for n in names:
        seen = run_config(m, n)
        new = missing(seen, table)
        print("%s: %d launches, %d not in the table" % (tag(n), len(seen), len(new)))
        print(describe_missing(new, table, limit=len(new)))
        if mode == "--write":
            rows = {key(r): r for r in table}
            for r in seen:
                if key(r) in rows:
                    if tag(n) not in rows[key(r)]["from"]:
                        rows[key(r)]["from"].append(tag(n))
                else:
                    table.append(dict(r, **{"from": [tag(n)]}))
    if mode == "--write":
        with open(TABLE, "w") as fh:
            for r in table:
                fh.write(json.dumps({k: r[k] for k in ("descs", "from", "lean", "tiles")}, sort_keys=True, separators=(",", ":")) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:] or ["--diff", "bf16_224", "fp32_224"])
