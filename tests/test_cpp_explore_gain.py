"""occupancy_grid::frontier_centres / explore_goals_by_gain and planner::gain_weight through the C++ successor header
(tests/cpp/test_explore_gain.cpp, linked with the C statement tests/cpp/explore_gain_ref.c): the program compiles as C++17 and
C++20 and fails loudly without a GPU; on the GPU it checks the two header calls against the C statement on the two-room map,
the planner with gain_weight = 0 (the goals of a planner without the member) and with gain_weight > 0 (the goal and heading of
the C statement), std::logic_error without line_of_sight, and prints OK."""
import os
import subprocess

import pytest

import sea_current_amd as sc

CPP = os.path.join(sc.REPO_ROOT, "tests", "cpp")
SRC = os.path.join(CPP, "test_explore_gain.cpp")
STATEMENT = [os.path.join(CPP, f) for f in ("explore_gain_ref.c", "sectors_ref.c", "views_ref.c")]


def _build(tmp_path, std):
    sc.build()
    objs = []
    for src in STATEMENT:
        objs.append(str(tmp_path / (os.path.basename(src)[:-2] + ".o")))
        subprocess.check_call(["cc", "-O2", "-std=c11", "-Wall", "-c", "-o", objs[-1], src])
    exe = str(tmp_path / f"test_explore_gain_{std}")
    subprocess.check_call(["g++", f"-std={std}", "-O1", "-Wall", "-Werror=return-type", "-o", exe, SRC, *objs,
                           "-L", sc.NATIVE_DIR, "-lsea_current_hip", f"-Wl,-rpath,{sc.NATIVE_DIR}"])
    return exe


@pytest.mark.parametrize("std", ["c++17", "c++20"])
def test_explore_gain_program_compiles(tmp_path, std):
    import torch
    exe = _build(tmp_path, std)
    if not torch.cuda.is_available():        # without a GPU the program must say so and fail
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode != 0
        assert "no CPU fallback" in r.stderr


@pytest.mark.gpu
def test_explore_gain_program_on_gpu(tmp_path):
    exe = _build(tmp_path, "c++20")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "explore_gain OK" in r.stdout
