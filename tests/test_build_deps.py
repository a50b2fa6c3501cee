"""libcpt.so's build inputs (cpppathtracer_amd/build.py) follow what is on disk: the rebuild
dependencies are every file under csrc/ (generated tables such as cpt_fm_tables.hpp included) and
the public header, and every translation unit in csrc/ is compiled."""
import os

from cpppathtracer_amd import build


def _csrc_files():
    return {os.path.join(root, f) for root, _, files in os.walk(build.CSRC) for f in files}


def test_deps_cover_csrc_and_public_header():
    deps = set(build.build_deps())
    assert os.path.join(build.CSRC, "cpt_fm_tables.hpp") in deps
    assert _csrc_files() <= deps
    assert os.path.join(build.REPO_DIR, "include", "cpt.h") in deps


def test_sources_are_the_translation_units_on_disk():
    units = {f for f in _csrc_files() if f.endswith((".hip", ".cpp"))}
    assert len(build.SOURCES) == len(set(build.SOURCES))
    assert set(build.SOURCES) == units
