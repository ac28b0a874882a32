#!/usr/bin/env python
"""What a kernel's machine code holds in flight: the order of vector-memory loads, vmcnt waits and MFMAs per kernel instance.

The lean kernel families rest on a wave requesting its operands before its first MFMA.  Whether it does is a
property of the instruction stream the compiler emitted, not of the source: the scheduler is free to sink loads between the MFMAs.
This tool compiles one .hip file for gfx950 with the flags of spann3r_amd/build.py, disassembles the device code object and prints,
per kernel instance:

  loads16        16-byte vector loads in the stream            before_mfma   16-byte loads ahead of the first MFMA
  max_in_flight  the longest run of outstanding loads, from a linear walk: +1 per vector load, a wait vmcnt(n) caps it at n
                 (vmcnt is a 6-bit count: it must stay <= 63)
  seq            the compact stream: L<n> = n loads in a row (l<n>: narrower than 16 bytes), W<n> = s_waitcnt vmcnt(n), M<n> = n MFMAs
  vgprs / agprs / scratch / occupancy from the compiler's resource remarks, and a hash of the load / wait / MFMA stream (two builds
  whose hash agrees issue the same stream)

It looks at load, wait and MFMA mnemonics only; the walk is linear, so inside a loop that was not unrolled the counts are those
of one trip.  No GPU is needed.

  python tools/issue_order.py spann3r_amd/csrc/gemm_sm.hip --kernel '^sm_kernel<' [--define NAME=VALUE] [--wide 160]"""
import argparse
import hashlib
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LOAD = re.compile(r"^(global|buffer|flat|scratch)_load_(\w+)")
WAIT = re.compile(r"^s_waitcnt\b(.*)")
VMCNT = re.compile(r"vmcnt\((\d+)\)")
MFMA = re.compile(r"^v_(s?mfma)\w*")
SYMBOL = re.compile(r"^[0-9a-f]+ <([^>]+)>:\s*$")


def parse_disassembly(text):
    """llvm-objdump -d text -> {symbol: [(kind, value)]}: ("L", bytes) per vector load, ("W", n) per wait that names vmcnt (a bare
    `s_waitcnt lgkmcnt(..)` does not touch it), ("M", 1) per MFMA, in program order"""
    out, cur = {}, None
    for line in text.splitlines():
        m = SYMBOL.match(line.strip())
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        ins = line.split("//")[0].strip()
        if not ins:
            continue
        m = LOAD.match(ins)
        if m:
            w = m.group(2)
            nbytes = 16 if "dwordx4" in w else 12 if "dwordx3" in w else 8 if "dwordx2" in w else 4 if "dword" in w else 2 if "short" in w else 1
            cur.append(("L", nbytes))
            continue
        m = WAIT.match(ins)
        if m:
            v = VMCNT.search(m.group(1))
            if v:
                cur.append(("W", int(v.group(1))))
            continue
        if MFMA.match(ins):
            cur.append(("M", 1))
    return out


def summarize(seq):
    """-> dict(loads16, loads, before_mfma, before_mfma_all, mfmas, max_in_flight, seq, hash) of one kernel's event list"""
    loads16 = sum(1 for k, v in seq if k == "L" and v == 16)
    loads = sum(1 for k, _ in seq if k == "L")
    first = next((i for i, (k, _) in enumerate(seq) if k == "M"), len(seq))
    before16 = sum(1 for k, v in seq[:first] if k == "L" and v == 16)
    before = sum(1 for k, _ in seq[:first] if k == "L")
    fly = peak = 0
    for k, v in seq:
        if k == "L":
            fly += 1
            peak = max(peak, fly)
        elif k == "W":
            fly = min(fly, v)
    parts, i = [], 0
    while i < len(seq):
        k, v = seq[i]
        if k == "W":
            parts.append("W%d" % v)
            i += 1
            continue
        tag = "M" if k == "M" else ("L" if v == 16 else "l")
        j = i
        while j < len(seq) and seq[j][0] == k and (k == "M" or (seq[j][1] == 16) == (v == 16)):
            j += 1
        parts.append("%s%d" % (tag, j - i))
        i = j
    text = " ".join(parts)
    return dict(loads16=loads16, loads=loads, before_mfma=before16, before_mfma_all=before, mfmas=sum(1 for k, _ in seq if k == "M"),
                max_in_flight=peak, seq=text, hash=hashlib.sha256(text.encode()).hexdigest()[:12])


REMARK = re.compile(r"remark:\s+(.*?)(?:\s+\[-Rpass[^\]]*\])?\s*$")


def parse_remarks(text):
    """-Rpass-analysis=kernel-resource-usage output -> {symbol: {vgprs, agprs, scratch, occupancy, lds}}"""
    out, cur = {}, None
    keys = {"VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "occupancy",
            "LDS Size [bytes/block]": "lds", "SGPRs": "sgprs"}
    for line in text.splitlines():
        m = REMARK.search(line)
        if not m:
            continue
        body = m.group(1).strip()
        if body.startswith("Function Name:"):
            cur = out.setdefault(body.split(":", 1)[1].strip(), {})
        elif cur is not None and ":" in body:
            k, v = body.rsplit(":", 1)
            if k.strip() in keys and v.strip().isdigit():
                cur[keys[k.strip()]] = int(v)
    return out


def demangle(names):
    import shutil
    filt = shutil.which("llvm-cxxfilt", path=os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")) or shutil.which("c++filt")
    if not names:
        return {}
    if not filt:
        return {n: n for n in names}
    try:
        # (binutils' c++filt does not know DF16b, the mangling of __bf16: hand it the vendor-type spelling of the same name)
        res = subprocess.run([filt] + [n.replace("DF16b", "u6__bf16") for n in names], stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()
        return dict(zip(names, res))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def compile_and_disassemble(src, defines=(), extra=()):
    """-> (disassembly text, resource remarks text)"""
    sys.path.insert(0, REPO)
    from spann3r_amd import build as B
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    hipcc = os.environ.get("HIPCC", os.path.join(rocm, "bin", "hipcc"))
    with tempfile.TemporaryDirectory() as tmp:
        co = os.path.join(tmp, "device.co")
        cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-x", "hip", "-c", src, "--cuda-device-only", "--no-gpu-bundle-output",
               "-o", co, "-Rpass-analysis=kernel-resource-usage", "-I", B.CSRC] + B.DEVICE_FLAGS + ["-D" + d for d in defines] + list(extra)
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        remarks = p.stdout.decode(errors="replace")
        if p.returncode != 0:
            sys.stderr.write(remarks)
            raise RuntimeError("hipcc failed on %s" % src)
        dis = subprocess.run([os.path.join(rocm, "llvm", "bin", "llvm-objdump"), "-d", co], stdout=subprocess.PIPE, check=True).stdout.decode()
    return dis, remarks


def report(dis, remarks, pattern=None, wide=150, out=sys.stdout):
    kernels = parse_disassembly(dis)
    res = parse_remarks(remarks)
    names = demangle(sorted(kernels))
    rows = sorted((names[s].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0], s) for s in kernels)
    for nice, sym in rows:
        if pattern and not re.search(pattern, nice):
            continue
        if res and sym not in res:                 # (device functions that were not inlined, if any: no resource remark)
            continue
        s, r = summarize(kernels[sym]), res.get(sym, {})
        out.write("%s\n" % nice)
        out.write("  loads16 %d (all loads %d)  before_mfma %d (all %d)  mfmas %d  max_in_flight %d  vgprs %d  agprs %d  scratch %d  occupancy %d  stream %s\n"
                  % (s["loads16"], s["loads"], s["before_mfma"], s["before_mfma_all"], s["mfmas"], s["max_in_flight"], r.get("vgprs", -1), r.get("agprs", -1),
                     r.get("scratch", -1), r.get("occupancy", -1), s["hash"]))
        words, line = s["seq"].split(), "  seq"
        for w in words:
            if len(line) + 1 + len(w) > wide:
                out.write(line + "\n")
                line = "     "
            line += " " + w
        out.write(line + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("source", help="a .hip file of spann3r_amd/csrc (or any HIP source)")
    ap.add_argument("--kernel", default=None, help="regular expression on the demangled kernel name")
    ap.add_argument("--define", action="append", default=[], help="NAME[=VALUE] passed as -D (repeatable)")
    ap.add_argument("--wide", type=int, default=150, help="line width of the sequence")
    ap.add_argument("--from-disassembly", default=None, help="parse this llvm-objdump -d text instead of compiling")
    ap.add_argument("--remarks", default=None, help="with --from-disassembly: the compiler's resource remarks (without: registers print as -1)")
    a = ap.parse_args()
    if a.from_disassembly:
        report(open(a.from_disassembly).read(), open(a.remarks).read() if a.remarks else "", a.kernel, a.wide)
        return
    dis, remarks = compile_and_disassemble(a.source, a.define)
    report(dis, remarks, a.kernel, a.wide)


if __name__ == "__main__":
    main()
