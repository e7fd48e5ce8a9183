"""CPU: saro-gs_amd/build.py -- what makes the library stale, and that its translation units cover csrc/ with every kernel compiled once.
Paths and file times are stand-ins in a temporary directory; the compiler is never run."""
import glob
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "saro-gs_amd", "csrc")
HEADERS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*.h")))
UNITS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*.hip")))


@pytest.fixture(scope="module")
def build_py():
    spec = importlib.util.spec_from_file_location("gsrast_build_under_test", os.path.join(ROOT, "saro-gs_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture
def stand_in(build_py, tmp_path, monkeypatch):
    """A tree of empty files under the real names, all older than the library beside them; -> (set_time(path, seconds from the library's), paths)."""
    src = tmp_path / "csrc"
    src.mkdir()
    t_out = os.path.getmtime(os.path.join(ROOT, "saro-gs_amd", "build.py")) + 1000.0      # (build.py itself is a dependency: the library is younger)
    paths = {n: str(src / n) for n in HEADERS + UNITS}
    paths["gsrast.h"], paths["out"] = str(tmp_path / "gsrast.h"), str(tmp_path / "libgsrast_hip.so")

    def set_time(name, dt):
        os.utime(paths[name], (t_out + dt, t_out + dt))
    for n in paths:
        open(paths[n], "w").close()
        set_time(n, 0.0 if n == "out" else -100.0)
    monkeypatch.setattr(build_py, "SRC_DIR", str(src))
    monkeypatch.setattr(build_py, "INCLUDE", paths["gsrast.h"])
    monkeypatch.setattr(build_py, "OUT", paths["out"])
    return set_time, paths


def test_up_to_date_library_is_kept(build_py, stand_in):
    assert HEADERS and "gsrast_distort.h" in HEADERS
    assert not build_py.needs_build()


@pytest.mark.parametrize("newer", HEADERS + UNITS + ["gsrast.h"])
def test_any_newer_source_makes_the_library_stale(build_py, stand_in, newer):
    set_time, _ = stand_in
    set_time(newer, +100.0)
    assert build_py.needs_build(), newer


def test_missing_library_is_stale(build_py, stand_in):
    os.remove(stand_in[1]["out"])
    assert build_py.needs_build()


def test_every_unit_is_a_source(build_py):
    assert UNITS and sorted(build_py.SOURCES) == UNITS


def _included(name, seen):
    """`seen` grows by every csrc header `name` includes, directly or through another."""
    for h in re.findall(r'^\s*#include\s+"(gsrast_\w+\.h)"', open(os.path.join(CSRC, name)).read(), flags=re.M):
        if h not in seen:
            seen.add(h)
            _included(h, seen)
    return seen


def test_every_kernel_header_is_compiled_in_exactly_one_unit(build_py):
    kernel_headers = [h for h in HEADERS if "__global__" in open(os.path.join(CSRC, h)).read()]
    assert len(kernel_headers) >= 16
    reach = {u: _included(u, set()) for u in build_py.SOURCES}
    for h in kernel_headers:
        units = [u for u in build_py.SOURCES if h in reach[u]]
        assert len(units) == 1, (h, units)
