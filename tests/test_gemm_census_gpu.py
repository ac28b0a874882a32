"""Replay of the launch census: every row of tests/golden/gemm_plan_table.jsonl -- every distinct auto-tile GEMM launch the model
issues -- is built by tests/gemm_desc_ref.py (guard bands, poisoned slack, non-minimal strides), launched with tile = -1 through
sp3_gemm / sp3_gemm_n, and every output compared with the float64 reference of the descriptor: whole-output max norm AND per problem
and 32-column group; a bf16 convolution output also per element, within half a bf16 step (gemm_desc_ref.conv_bf16_excess: a half-resolution
res2 may round to either bf16 neighbour where its float64 value lies within the fp32 interpolation bound of a rounding boundary, on at
most 1 % of a row).  The plan of the real descriptor must still be the recorded tile.  Rows recorded with the lean instances off run
in one child process (SP3_LEAN_GEMM is read once per process).  test_census_is_current keeps the table honest: a model launch that is
not a row of it fails there."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

import gemm_desc_ref as R

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(REPO, "tests", "golden", "gemm_plan_table.jsonl")
ROWS = [(i + 1, json.loads(line)) for i, line in enumerate(open(TABLE))]
# rows the replay does not cover, by line of the table -- tests/test_gemm_desc_ref_cpu.py pins this list and its reasons
NOT_COVERED = {
    197: "tile 45, score stage of the long-bank read: p~ = exp(s - group max) in fragment order with 64-key group statistics "
         "([ldc / 64][rows_pad] layout) -- not restated; test_long_bank_read_without_a_score_matrix covers it with its consumer",
    198: "tile 46, P.V stage of the long-bank read: fragment-order p~ with the merged group scales in sm_stats -- not restated",
}


def _flops(row):
    return sum(2.0 * d["M"] * d["N"] * d["K"] * max(d.get("batch", 1), 1) for d in row["descs"])


def _id(line, row):
    return "L%d-%s-t%s" % (line, row["from"][0], "+".join(str(t) for t in row["tiles"]))


def replay_row(line, row, report=None):
    """builds, launches and checks one row; returns the list of failures (empty = pass)"""
    import torch
    from spann3r_amd import lib as L
    l = L.load()
    fails = []
    for dyn in R.dyn_extents(row):
        cases = [c.materialize("cuda") for c in R.row_cases(row, line, dyn)]
        ds = [c.desc(L) for c in cases]
        if len(ds) == 1:
            tiles = [int(l.sp3_gemm_plan(C.byref(ds[0])))]
        else:
            arr = (C.POINTER(L.GemmDesc) * len(ds))(*[C.pointer(d) for d in ds])
            t = (C.c_int * len(ds))()
            tiles = list(t) if l.sp3_gemm_plan_n(arr, len(ds), t) == 0 else [-1] * len(ds)
        if tiles != row["tiles"]:
            fails.append("plan %r, table %r" % (tiles, row["tiles"]))
            continue                                  # (never launched on an instance the row was not recorded on)
        torch.cuda.synchronize()
        if len(ds) == 1:
            L.check(l.sp3_gemm(C.byref(ds[0]), L.stream_ptr()), "sp3_gemm")
        else:
            L.check(l.sp3_gemm_n(arr, len(ds), L.stream_ptr()), "sp3_gemm_n")
        torch.cuda.synchronize()
        for i, c in enumerate(cases):
            f, errs = R.compare(c)
            fails += ["desc %d%s: %s" % (i, "" if dyn is None else " (extent %d)" % dyn, s) for s in f]
            if report is not None:
                report.append({"line": line, "tile": row["tiles"][i], "lean": row["lean"], "errs": errs, "ok": not f, "fails": f})
        del cases, ds
    return fails


def _dump(report):
    path = os.environ.get("SP3_CENSUS_REPORT")
    if path:
        with open(path, "a") as fh:
            for r in report:
                fh.write(json.dumps(r) + "\n")


LEAN_ON = sorted(((ln, r) for ln, r in ROWS if r["lean"] == 1 and ln not in NOT_COVERED), key=lambda x: _flops(x[1]))
LEAN_OFF = sorted(((ln, r) for ln, r in ROWS if r["lean"] == 0 and ln not in NOT_COVERED), key=lambda x: _flops(x[1]))


@pytest.mark.parametrize("line,row", LEAN_ON, ids=[_id(ln, r) for ln, r in LEAN_ON])
def test_census_row(line, row):
    assert os.environ.get("SP3_LEAN_GEMM", "1")[:1] != "0"
    report = []
    fails = replay_row(line, row, report)
    _dump(report)
    assert not fails, "\n".join(fails)


def _child():
    """all rows recorded with the lean instances off, in this one process; one JSON line per row"""
    report = []
    for line, row in LEAN_OFF:
        fails = replay_row(line, row, report)
        print(json.dumps({"id": _id(line, row), "fails": fails}), flush=True)
    _dump(report)
    print("rows %d" % len(LEAN_OFF), flush=True)


def test_census_rows_lean_instances_off():
    assert len(LEAN_OFF) > 50
    env = dict(os.environ, SP3_LEAN_GEMM="0", PYTHONPATH=os.pathsep.join([REPO, os.path.join(REPO, "tests"), os.environ.get("PYTHONPATH", "")]))
    out = subprocess.run([sys.executable, "-c", "import test_gemm_census_gpu as t; t._child()"], env=env, capture_output=True, text=True, timeout=900)
    res = [json.loads(s) for s in out.stdout.splitlines() if s.startswith("{")]
    assert out.returncode == 0 and ("rows %d" % len(LEAN_OFF)) in out.stdout, "after %d rows: %s" % (len(res), out.stdout[-2000:] + out.stderr[-4000:])
    bad = [r for r in res if r["fails"]]
    assert not bad, "\n".join("%s: %s" % (r["id"], "; ".join(r["fails"])) for r in bad)


def test_every_row_is_replayed_or_listed():
    assert len(LEAN_ON) + len(LEAN_OFF) + len(NOT_COVERED) == len(ROWS) == 605


def test_census_is_current(full_sd):
    """the launches of the bf16 and fp32 224 x 224 configurations (at the frame counts the table was taken with) are rows of the table: a
    model change that adds a launch the replay has never seen fails here, next to the row it differs least from (tools/gemm_census.py
    --write adds it)"""
    from spann3r_amd import Spann3R, FULL
    from tools import gemm_census
    m = Spann3R(dus3r_name=None, cfg=FULL, init_weights=False)
    m.load_state_dict(full_sd, strict=True)
    m = m.to("cuda").eval()
    table = gemm_census.load_table()
    for name in ("bf16_224", "fp32_224"):
        seen = gemm_census.run_config(m, name)
        assert len(seen) > 30, (name, len(seen))
        new = gemm_census.missing(seen, table)
        assert not new, "%s: %d of %d launches are not in the census:\n%s" % (name, len(new), len(seen), gemm_census.describe_missing(new, table))
