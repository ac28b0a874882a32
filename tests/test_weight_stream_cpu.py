"""The weight cache policy (sp3_weight_stream_set, SP3_W_STREAM; csrc/weight_stream.cpp) is no part of launch planning: for every row
of tests/golden/gemm_plan_table.jsonl the planned tiles are the recorded ones under modes 0 (default policy everywhere), 1 (the
library's table) and 2 (every streaming variant).  Host code only: no GPU."""
import json
import os
import subprocess
import sys

import pytest

import test_gemm_plan_cpu as P

REPO = P.REPO
MODES = (0, 1, 2)


def _set(mode):
    from spann3r_amd import lib
    l = lib.load()
    assert l.sp3_weight_stream_set(mode) == 0 and l.sp3_weight_stream_get() == mode


def _check_all_modes(lean):
    """rows checked per mode; the mode is put back to what the process had"""
    from spann3r_amd import lib
    before = lib.load().sp3_weight_stream_get()
    try:
        counts = []
        for mode in MODES:
            _set(mode)
            counts.append(P._check_table(lean))
    finally:
        _set(before)
    return counts


def test_mode_entry_point():
    from spann3r_amd import lib
    l = lib.load()
    before = l.sp3_weight_stream_get()
    assert before in MODES
    for bad in (-1, 3):
        assert l.sp3_weight_stream_set(bad) != 0 and b"sp3_weight_stream_set" in l.sp3_last_error()
        assert l.sp3_weight_stream_get() == before


@pytest.mark.parametrize("value,mode", [("0", 0), ("1", 1), ("2", 2), (None, 1), ("x", 1)])
def test_mode_from_environment(value, mode):
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("SP3_W_STREAM", None)
    if value is not None:
        env["SP3_W_STREAM"] = value
    out = subprocess.run([sys.executable, "-c", "from spann3r_amd import lib; print('mode', lib.load().sp3_weight_stream_get())"],
                         env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and ("mode %d" % mode) in out.stdout, out.stdout + out.stderr


def test_plan_table_every_mode_lean_instances_on():
    assert os.environ.get("SP3_LEAN_GEMM", "1")[:1] != "0"
    counts = _check_all_modes(1)
    assert len(set(counts)) == 1 and counts[0] > 50


def test_plan_table_every_mode_lean_instances_off():
    """SP3_LEAN_GEMM is read once per process: the rows recorded with the lean instances off are planned in a child process"""
    rows = [json.loads(line) for line in open(P.TABLE)]
    n_off = sum(1 for r in rows if r["lean"] == 0)
    env = dict(os.environ, SP3_LEAN_GEMM="0", PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    code = "import sys; sys.path.insert(0, %r); import test_weight_stream_cpu as t; print('rows', t._check_all_modes(0))" % os.path.join(REPO, "tests")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and ("rows [%d, %d, %d]" % (n_off, n_off, n_off)) in out.stdout, out.stdout + out.stderr
