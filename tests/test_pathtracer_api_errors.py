"""What PathTracer answers before it has a camera, a frame or a context, with no GPU: a small C++
program on the drop-in header.  Every call here is refused before it reaches a device, with an
exact return value and an exact LastError(); a refused call that sets no message leaves the last
one standing.  The camera check comes before the implicit BuildBVH, so none of the calls builds.
(SetDevices(n >= 1) is not called: it asks HIP for its device count.)"""
import os
import subprocess

from cpppathtracer_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <cstdio>
#include <string>
#include <vector>

#include "cpppathtracer/path_tracer.h"

static int bad = 0;
static void expect(bool ok, const char* what) {
    if (!ok) { printf("FAILED: %s\n", what); ++bad; }
}
static void expect_error(const PathTracer& t, const std::string& want) {
    if (t.LastError() != want) { printf("FAILED: LastError \"%s\", expected \"%s\"\n", t.LastError().c_str(), want.c_str()); ++bad; }
}

int main() {
    PathTracer t;
    std::vector<float> rgb, depth, normal, albedo;
    std::vector<int32_t> id;
    std::vector<uint8_t> bgra;
    float rel[1];
    cpt_stats stats;
    const MotionalCamera from(16, 16);

    expect(t.LastError().empty(), "a fresh tracer has no error");
    // no message of their own: the error stays as it was (empty here)
    expect(!t.ReadFrameBGRA(bgra), "ReadFrameBGRA");
    expect(!t.GetStats(&stats), "GetStats on a fresh tracer");
    expect(!t.GetStats(nullptr), "GetStats(nullptr)");
    expect(t.SetMaxRecursionDepth(32), "SetMaxRecursionDepth(32)");
    expect_error(t, "");

    // the calls that need a camera
    expect(!t.Render(1, false), "Render");
    expect_error(t, "Render: SetCamera first");
    expect(SceneBVH::BuildId() == 0, "Render without a camera does not build");
    expect(!t.RenderToCount(2), "RenderToCount");
    expect_error(t, "RenderToCount: SetCamera first");
    expect(!t.RenderAdaptive(2, 4, 2, 0.1f), "RenderAdaptive");
    expect_error(t, "RenderAdaptive: SetCamera first");
    expect(!t.ReadGBuffer(id, depth, normal, albedo), "ReadGBuffer");
    expect_error(t, "ReadGBuffer: SetCamera first");
    expect(!t.Reproject(from), "Reproject");
    expect_error(t, "Reproject: SetCamera first");
    expect(!t.CaptureHistory(), "CaptureHistory");
    expect_error(t, "CaptureHistory: SetCamera first");
    expect(!t.ReprojectTracked(), "ReprojectTracked");
    expect_error(t, "ReprojectTracked: SetCamera first");
    expect(SceneBVH::BuildId() == 0, "ReprojectTracked without a camera does not build");
    expect(t.Pick(0, 0) == -1, "Pick");
    expect_error(t, "Pick: SetCamera first");
    expect(SceneBVH::BuildId() == 0, "no call without a camera builds");

    // still no message of their own: Pick's stays
    expect(!t.ReadFrameBGRA(bgra), "ReadFrameBGRA after an error");
    expect(!t.GetStats(&stats), "GetStats after an error");
    expect(!t.GetStats(nullptr), "GetStats(nullptr) after an error");
    expect_error(t, "Pick: SetCamera first");

    // the readers and filters that need a frame
    expect(!t.ReadNoise(rel), "ReadNoise");
    expect_error(t, "ReadNoise: RenderAdaptive first");
    expect(!t.FilterRadiance(), "FilterRadiance");
    expect_error(t, "FilterRadiance: RenderAdaptive first");
    expect(!t.FilterRadianceSpatial(), "FilterRadianceSpatial");
    expect_error(t, "FilterRadianceSpatial: Render first");
    expect(!t.ReadFiltered(rgb), "ReadFiltered");
    expect_error(t, "ReadFiltered: FilterRadiance first");
    expect(!t.ReadRadiance(rgb), "ReadRadiance");
    expect_error(t, "ReadRadiance: nothing rendered");
    expect(!t.SaveFilteredPFM("unwritten.pfm"), "SaveFilteredPFM");
    expect_error(t, "ReadFiltered: FilterRadiance first");
    expect(!t.SaveRadiancePFM("unwritten.pfm"), "SaveRadiancePFM");
    expect_error(t, "ReadRadiance: nothing rendered");

    // the setters
    expect(!t.SetMaxRecursionDepth(33), "SetMaxRecursionDepth(33)");
    expect_error(t, "SetMaxRecursionDepth: depth must be <= 32");
    expect(t.SetMaxRecursionDepth(32), "SetMaxRecursionDepth(32) after a refusal");
    expect_error(t, "SetMaxRecursionDepth: depth must be <= 32");
    expect(!t.SetDevices(std::vector<int>{}), "SetDevices({})");
    expect_error(t, "SetDevices: empty device list");
    expect(!t.SetDevices(0), "SetDevices(0)");
    expect_error(t, "SetDevices: n must be >= 1");
    printf("bad %d\n", bad);
    return bad != 0;
}
"""


def test_calls_before_camera_and_frame_are_refused_with_their_messages(tmp_path):
    src, exe = tmp_path / "errors.cpp", tmp_path / "errors"
    src.write_text(SRC)
    lib = _lib.lib_path()
    assert os.path.exists(lib), lib
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src), lib,
                    "-Wl,-rpath," + os.path.dirname(lib)], check=True)
    r = subprocess.run([str(exe)], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "bad 0" in r.stdout, r.stdout + r.stderr
    assert not (tmp_path / "unwritten.pfm").exists()
