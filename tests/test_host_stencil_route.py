"""CPU-side check of the C++ facade's routing policy (tests/host/stencil_route.cpp): Stencil2D::resolve_route -- which arrays and which C entry
point serve an apply -- against a table written out by hand, on fabricated states, and the plan of one vector through the masked entry point
against qmg_stencil_apply's on the fp64 rows of the stencil route table.  Compiled with g++ (address and undefined-behaviour sanitizers on: a
stand-alone host program) against the headers; libqmg_hip.so is linked for its symbols only -- no GPU call is made."""
import importlib
import os
import subprocess

import test_gpu_stencil_routes as routes

qmg = importlib.import_module("quantum-mg_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_facade_stencil_route(tmp_path):
    qmg.build()
    libdir = os.path.join(ROOT, "quantum-mg_amd")
    exe = str(tmp_path / "stencil_route")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++11", "-Wall", "-Wno-unused-variable", "-Wno-unused-parameter", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(ROOT, "tests", "host", "stencil_route.cpp"), "-L" + libdir, "-lqmg_hip", "-Wl,-rpath," + libdir])
    requests = sorted({(row[2], routes.PIECES[row[5]]) for row in routes.ROUTES if row[1] == "c64"})
    assert len(requests) > 20
    args = [str(v) for (dims, pieces) in requests for v in (*dims, pieces)]
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "stencil route ok" in out.stdout
    assert "%d plan pairs" % (8 * len(requests)) in out.stdout
