"""CPU checks of the polygon rasterisation rule (sc_occ_from_polygons): the numpy twin tests/occ_twin.py equals the
successor header's host occupancy_grid::rasterize / planning_space::make_grid(), byte for byte, on every world the GPU
tests use (tests/cpp/rasterize_dump.cpp writes the header's bytes; it creates no gpu_context).  No GPU needed."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import sea_current_amd as sc
import occ_twin as tw

SRC = os.path.join(sc.REPO_ROOT, "tests", "cpp", "rasterize_dump.cpp")


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    sc.build()
    d = tmp_path_factory.mktemp("rasterize_dump")
    exe = str(d / "rasterize_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror=return-type", "-o", exe, SRC, "-L", sc.NATIVE_DIR,
                           "-lsea_current_hip", f"-Wl,-rpath,{sc.NATIVE_DIR}"])

    def run(worlds):
        outs = [str(d / f"w{i}.occ") for i in range(len(worlds))]
        spec = str(d / "worlds.txt")
        tw.write_worlds(spec, worlds, outs)
        subprocess.check_call([exe, spec])
        return [tw.read_dump(o) for o in outs]
    return run


def _check(dump, worlds):
    for name, host in zip(worlds, dump(list(worlds.values()))):
        w = worlds[name]
        assert host.shape == (w["frame"][1], w["frame"][0]), name
        twin = tw.rasterize_world(w)
        assert np.array_equal(twin, host), (name, int((twin != host).sum()))


def test_twin_equals_header_on_special_worlds(dump):
    worlds = tw.special_worlds()
    worlds["poly14_4096"] = tw.polygon_world(4096)
    worlds["left60_1024"] = tw.left60_world(1024)
    worlds["left60_700"] = tw.left60_world(700)
    worlds["poly14_1000"] = tw.polygon_world(1000)
    _check(dump, worlds)


def test_twin_equals_header_on_random_worlds(dump):
    _check(dump, {f"random_{s}": tw.random_world(s) for s in range(0, 300, 3)})


def test_twin_marks_something(dump):
    """The worlds are not trivially empty or full: fill and edges both matter."""
    w = tw.polygon_world(1024)
    occ = tw.rasterize_world(w)
    assert 0.02 < occ.mean() < 0.5
    L, off, cl, bx = tw.flatten(w["obstacles"])
    edges_only = tw.rasterize(w["frame"], L, off, np.zeros_like(cl), bx)
    assert 0 < edges_only.sum() < occ.sum()


def test_polygons_declared_and_exported():
    sc.build()
    lib = ctypes.CDLL(sc.LIB_PATH)
    src = re.sub(r"/\*.*?\*/", "", open(sc.HEADER_PATH).read(), flags=re.S)
    for name in ("sc_occ_from_polygons", "sc_occ_from_polygons_host"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert hasattr(lib, name), name
        assert name in sc.EXPORTS, name
