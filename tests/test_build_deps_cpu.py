"""spann3r_amd.build._deps covers every header the library is built from: for every file of build.SOURCES, and transitively for
every header it includes, each `#include "name.h"` that resolves inside csrc/ is among the dependencies whose hash decides whether
the library is rebuilt.  Text parsing only; no compiler."""
import os
import re

from spann3r_amd import build

INCLUDE = re.compile(r'^\s*#\s*include\s+"([^"]+)"', re.M)


def _local_includes(path):
    with open(path) as f:
        names = INCLUDE.findall(f.read())
    return [os.path.normpath(os.path.join(os.path.dirname(path), n)) for n in names]


def test_every_included_csrc_header_is_a_dependency():
    csrc = os.path.normpath(build.CSRC)
    deps = {os.path.normpath(d) for d in build._deps()}
    todo, seen, edges = [os.path.join(csrc, s) for s in build.SOURCES], set(), 0
    while todo:
        path = todo.pop()
        if path in seen:
            continue
        seen.add(path)
        assert path in deps, "%s is compiled or included but is not in build._deps()" % os.path.relpath(path, csrc)
        for inc in _local_includes(path):
            if os.path.dirname(inc) == csrc and os.path.exists(inc):
                edges += 1
                todo.append(inc)
    headers = sorted(os.path.basename(p) for p in seen if p.endswith(".h"))
    print("sources", len(build.SOURCES), "headers reached", headers, "include edges", edges)
    assert len(seen) > len(build.SOURCES) and "slab.h" in headers and "tsdf.h" in headers      # the walk did find headers
