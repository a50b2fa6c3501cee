"""PathTracer::SetDisplayReprojection's argument check, with no GPU: a small C++
program on the drop-in header.  The call only stores its settings, so it reaches no device; what
cpt_reproject_display would refuse at every Refresh (max_history < 1, a negative or non-finite
plane_tol) it refuses once, with false and LastError, and a refused call changes nothing: the
error of the next refused call is that call's own, and valid calls go on succeeding."""
import os
import subprocess

from cpppathtracer_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <cmath>
#include <cstdio>
#include <string>

#include "cpppathtracer/path_tracer.h"

static int bad = 0;
static void expect(bool ok, const char* what) {
    if (!ok) { printf("FAILED: %s\n", what); ++bad; }
}

int main() {
    PathTracer t;
    expect(t.LastError().empty(), "a fresh tracer has no error");
    expect(t.SetDisplayReprojection(true), "the defaults are accepted");
    expect(t.SetDisplayReprojection(true, 1, 0.0f), "max_history 1 and plane_tol 0 are accepted");
    expect(t.LastError().empty(), "accepted calls leave no error");
    expect(!t.SetDisplayReprojection(true, 0), "max_history 0 is refused");
    expect(t.LastError().find("SetDisplayReprojection") == 0, "the error names the call");
    expect(t.LastError().find("max_history 0") != std::string::npos, "the error names the value");
    expect(!t.SetDisplayReprojection(true, -3), "a negative max_history is refused");
    expect(t.LastError().find("max_history -3") != std::string::npos, "the error is the last refused call's");
    expect(!t.SetDisplayReprojection(true, 32, -1e-2f), "a negative plane_tol is refused");
    expect(!t.SetDisplayReprojection(true, 32, NAN), "a NaN plane_tol is refused");
    expect(!t.SetDisplayReprojection(true, 32, INFINITY), "an infinite plane_tol is refused");
    expect(!t.SetDisplayReprojection(false, 0), "off does not excuse the arguments");
    expect(t.SetDisplayReprojection(false), "off with the defaults is accepted");
    expect(t.SetDisplayReprojection(true, 128, 1e-1f), "other valid settings are accepted");
    printf("bad %d\n", bad);
    return bad != 0;
}
"""


def test_set_display_reprojection_refuses_bad_arguments(tmp_path):
    src, exe = tmp_path / "sdr.cpp", tmp_path / "sdr"
    src.write_text(SRC)
    lib = _lib.lib_path()
    assert os.path.exists(lib), lib
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src), lib,
                    "-Wl,-rpath," + os.path.dirname(lib)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "bad 0" in r.stdout, r.stdout + r.stderr
