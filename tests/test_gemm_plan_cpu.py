"""Launch planning lives in the library (csrc/gemm.hip gemm_plan): sp3_gemm_plan / sp3_gemm_plan_n are host code, so the tile of
every hot-path descriptor is checked here without a GPU.

tests/golden/gemm_plan_table.jsonl is the census taken when the Python mirror of the heuristic was removed: every distinct
descriptor (and grouped launch) with tile < 0 that the model issues -- 224 x 224, 512 x 512 and batch 4 in bf16, fp32 and f16x3
operands, the whole-sequence encoder, the training step in bf16 and fp32, with the lean instances on and off -- next to the tile
the launch ran on at that commit.  Pointers are kept as set / not set, strides and byte offsets are dropped (no rule reads them).
A rule change shows up as a diff of this table."""
import ctypes as C
import itertools
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(REPO, "tests", "golden", "gemm_plan_table.jsonl")


def _desc(lib, fields):
    d = lib.GemmDesc()
    ptrs = {n for n, t in lib.GemmDesc._fields_ if t is C.c_void_p}
    for k, v in fields.items():
        setattr(d, k, 4096 if k in ptrs else v)
    d.tile = -1
    return d


def _plan(lib, fields_list):
    """tiles the library plans for one call of sp3_gemm_n (sp3_gemm for one descriptor) with these descriptors"""
    l = lib.load()
    ds = [_desc(lib, f) for f in fields_list]
    if len(ds) == 1:
        return [l.sp3_gemm_plan(C.byref(ds[0]))]
    arr = (C.POINTER(lib.GemmDesc) * len(ds))(*[C.pointer(d) for d in ds])
    tiles = (C.c_int * len(ds))()
    rc = l.sp3_gemm_plan_n(arr, len(ds), tiles)
    return list(tiles) if rc == 0 else [-1] * len(ds)


def _check_table(lean):
    from spann3r_amd import lib
    rows = [json.loads(line) for line in open(TABLE)]
    rows = [r for r in rows if r["lean"] == lean]
    assert len(rows) > 50
    bad = [(r["descs"], r["tiles"], got) for r in rows for got in [_plan(lib, r["descs"])] if got != r["tiles"]]
    assert not bad, "%d of %d plans differ, first: %r" % (len(bad), len(rows), bad[0])
    return len(rows)


def test_plan_table_lean_instances_on():
    assert os.environ.get("SP3_LEAN_GEMM", "1")[:1] != "0"
    _check_table(1)


def test_plan_table_lean_instances_off():
    """SP3_LEAN_GEMM is read once per process: the rows taken with the lean instances off are checked in a child process.  Among them
    the wide many-row GEMMs of the whole-sequence bf16 encoder (q/k/v and fc1 at 1960 rows) on the 128-row LDS-staged tiles."""
    rows = [json.loads(line) for line in open(TABLE)]
    wide = {r["descs"][0]["N"]: r["tiles"][0] for r in rows if r["lean"] == 0 and len(r["descs"]) == 1 and r["descs"][0]["M"] == 1960}
    assert wide[3072] in (5, 6) and wide[4096] == 5
    env = dict(os.environ, SP3_LEAN_GEMM="0", PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    code = "import sys; sys.path.insert(0, %r); import test_gemm_plan_cpu as t; print('rows', t._check_table(0))" % os.path.join(REPO, "tests")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "rows" in out.stdout, out.stdout + out.stderr


def _packed_bf16(lib, M, N, K, **kw):
    return dict(dict(A=1, W=1, C=1, bias=1, M=M, N=N, K=K, lda=K, ldc=N, alpha=1.0, a_bf16=1, a_packed=1, w_packed=1, wdtype=lib.BF16), **kw)


def test_group_plan_rules():
    from spann3r_amd import lib
    l = lib.load()
    wide, narrow = _packed_bf16(lib, 1024, 3072, 768, relu_in=1), _packed_bf16(lib, 1024, 768, 768, relu_in=1)    # (relu_in: general tiles only)
    tw, tn = _plan(lib, [wide])[0], _plan(lib, [narrow])[0]
    assert tw in (5, 6) and tn >= 20
    # a pair's second group runs on the first one's tile
    assert _plan(lib, [wide, narrow]) == [tw, tw] and _plan(lib, [narrow, wide]) == [tn, tn]
    # more than two groups: no member changes its instance -- a level whose members choose different tiles is refused ...
    assert _plan(lib, [wide, wide, narrow]) == [-1, -1, -1]
    assert b"one kernel instance" in l.sp3_last_error()
    ds = [_desc(lib, f) for f in (wide, wide, narrow)]
    arr = (C.POINTER(lib.GemmDesc) * 3)(*[C.pointer(d) for d in ds])
    assert l.sp3_gemm_n(arr, 3, None) != 0 and b"one kernel instance" in l.sp3_last_error()       # (refused before anything is launched)
    # ... and one whose members agree is planned on that tile
    assert _plan(lib, [wide, wide, wide, wide]) == [tw] * 4
    # a lean q/k/v pair shares positions and RoPE tables (header, sp3_gemm_n): planning reads no pointer values and answers the pair's
    # tile, the launch refuses two descriptors with different pos pointers -- before anything is launched
    rope = dict(epi=lib.EPI_ROPE_VT, heads=12, tokens=196, vt_ld=256, qkv_packed=1, pos=1, rope_cos=1, rope_sin=1, vt=1, ln_stats=1, ln_s=1,
                ln_nt=24, ln_C=768, batch=2)
    qkv, ckv = _packed_bf16(lib, 196, 2304, 768, rope_cols=1536, **rope), _packed_bf16(lib, 196, 1536, 768, rope_cols=768, **rope)
    if _plan(lib, [qkv])[0] >= 30:                      # (lean instances on)
        assert _plan(lib, [qkv, ckv]) == [31, 31]
        ds = [_desc(lib, f) for f in (qkv, ckv)]
        ds[1].pos = 8192
        arr = (C.POINTER(lib.GemmDesc) * 2)(*[C.pointer(d) for d in ds])
        tiles = (C.c_int * 2)()
        assert l.sp3_gemm_plan_n(arr, 2, tiles) == 0 and list(tiles) == [31, 31]
        assert l.sp3_gemm_n(arr, 2, None) != 0 and b"do not share a lean instance" in l.sp3_last_error()
    # different operand dtypes never share a launch
    f32 = dict(A=1, W=1, C=1, M=196, N=768, K=768, lda=768, ldc=768, alpha=1.0)
    assert _plan(lib, [f32, dict(f32, wdtype=lib.BF16)]) == [-1, -1]


def test_fp16_plane_weights_are_checked():
    """w_packed = 2 (fp16 planes in place of fp32 weights) is read by the f16x3 instances of tiles 0..2 only"""
    from spann3r_amd import lib
    l = lib.load()
    ok = dict(A=1, W=1, C=1, M=196, N=768, K=768, lda=768, ldc=768, alpha=1.0, w_packed=2, f32x3=4)
    assert _plan(lib, [ok]) == [0] and _plan(lib, [dict(ok, M=4096)]) == [1]
    for bad in (dict(ok, f32x3=0), dict(ok, f32x3=1), dict(ok, wdtype=lib.BF16),
                dict(ok, loader=lib.LOAD_SOFTMAX, sm_stats=1, sm_nt=24, lda=768)):
        assert _plan(lib, [bad]) == [-1], bad
        assert b"w_packed = 2" in l.sp3_last_error()
    d = _desc(lib, ok)
    d.tile = 3
    assert l.sp3_gemm(C.byref(d), None) != 0 and b"w_packed = 2" in l.sp3_last_error()


GENERAL_TILES = {0, 1, 2, 3, 5, 6, 13, 20, 21, 22, 24, 25}       # csrc/gemm.hip dispatch_tile: every general tile there is
PLANNED_TILES = {0, 1, 2, 5, 6, 13, 20, 21, 22, 24}              # ... and the ones gemm_prepare can answer (3 and 25: by number only)
REMOVED_TILES = (4, 18, 7, 8, 9, 10, 11, 12, 14, 15, 16, 17, 23)


def test_removed_tile_numbers_are_refused():
    """a tile number without a kernel instance answers like any unknown one, before anything is launched (null stream, no GPU)"""
    from spann3r_amd import lib
    l = lib.load()
    for fields in (dict(A=1, W=1, C=1, M=196, N=768, K=768, lda=768, ldc=768, alpha=1.0), _packed_bf16(lib, 1024, 768, 768)):
        for n in REMOVED_TILES + (19, 26, 29):
            d = _desc(lib, fields)
            d.tile = n
            assert l.sp3_gemm(C.byref(d), None) != 0, n
            assert b"bad tile %d" % n in l.sp3_last_error(), (n, l.sp3_last_error())


def test_planner_answers_existing_tiles_only():
    """gemm_prepare cannot choose a tile that dispatch_tile does not have: every census row and a grid of synthetic descriptors
    (fp32 and bf16, packed and row-major operands, plain and conv loader, split-K 1 and 8)"""
    from spann3r_amd import lib
    assert PLANNED_TILES <= GENERAL_TILES and not GENERAL_TILES & set(REMOVED_TILES)
    answers = []
    for r in map(json.loads, open(TABLE)):
        answers += [_plan(lib, [f])[0] for f in r["descs"]]
    assert len(answers) >= 605 and min(answers) >= 0
    for M, N, K in itertools.product((7, 196, 784, 1960, 4096, 16384), (96, 768, 2304, 4096, 16384), (64, 768, 4096)):
        for bf16, packed, conv, sk in itertools.product((0, 1), (0, 1), (0, 1), (1, 8)):
            f = dict(A=1, W=1, C=1, bias=1, M=M, N=N, K=K, lda=K, ldc=N, alpha=1.0, splitk=sk)
            if bf16:
                f.update(wdtype=lib.BF16, a_bf16=1)
            if packed:
                f.update(a_packed=1, w_packed=1)
            if sk > 1:
                f.update(epi=lib.EPI_PARTIAL)
            if conv:                                    # K = 9 Cin, M = one OH x OW map per 49 rows (invalid combinations answer -1)
                f.update(loader=lib.LOAD_CONV3X3, conv_C=K // 9, conv_H=7, conv_W=7, conv_OH=7, conv_OW=7, conv_stride=1)
            answers.append(_plan(lib, [f])[0])
    got = {t for t in answers if 0 <= t < 30}
    assert sum(1 for t in answers if t >= 0) > 700 and got <= PLANNED_TILES, sorted(got - PLANNED_TILES)
    assert got >= {0, 1, 2, 5, 6, 20, 22, 24}, sorted(got)       # (the sweep does reach the rules' arms)
