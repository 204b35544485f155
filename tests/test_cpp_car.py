"""car_model, occupancy_grid::arc_mask / car_fields / car_paths and the car_model overload of planning_space::plan_to_pose
through the C++ successor header (tests/cpp/test_car.cpp): the program compiles as C++17 and C++20 and fails loudly without a
GPU; on the GPU it checks the arc mask against the definition restated on the host and plan_to_pose on the two-room map against
a host Dijkstra over the car graph restated in the program -- the first pose is the start, the last the goal pose, the entries
read as legal edges whose costs add up to the optimum, no two consecutive entries share a cell, no path for a body wider than
the door -- and prints OK."""
import os
import subprocess

import pytest

import sea_current_amd as sc

SRC = os.path.join(sc.REPO_ROOT, "tests", "cpp", "test_car.cpp")


def _build(tmp_path, std):
    sc.build()
    exe = str(tmp_path / f"test_car_{std}")
    subprocess.check_call(["g++", f"-std={std}", "-O1", "-Wall", "-Werror=return-type", "-o", exe, SRC,
                           "-L", sc.NATIVE_DIR, "-lsea_current_hip", f"-Wl,-rpath,{sc.NATIVE_DIR}"])
    return exe


@pytest.mark.parametrize("std", ["c++17", "c++20"])
def test_car_program_compiles(tmp_path, std):
    import torch
    exe = _build(tmp_path, std)
    if not torch.cuda.is_available():        # without a GPU the program must say so and fail
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode != 0
        assert "no CPU fallback" in r.stderr


@pytest.mark.gpu
def test_car_program_on_gpu(tmp_path):
    exe = _build(tmp_path, "c++20")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "car OK" in r.stdout
