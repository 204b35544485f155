"""heading_dirs, occupancy_grid::known_from_sectors / sector_gain / view_gain_headings and planner::fov_span through the C++
successor header (tests/cpp/test_sectors.cpp): the program compiles as C++17 and C++20 and fails loudly without a GPU; on the
GPU it checks the three header calls against a host restatement on the two-room map, the planner with a quarter-circle sensor
behind a closed wall, std::logic_error without line_of_sight, and with fov_span = 0 the results of test_views.cpp's scenario,
and prints OK."""
import os
import subprocess

import pytest

import sea_current_amd as sc

SRC = os.path.join(sc.REPO_ROOT, "tests", "cpp", "test_sectors.cpp")


def _build(tmp_path, std):
    sc.build()
    exe = str(tmp_path / f"test_sectors_{std}")
    subprocess.check_call(["g++", f"-std={std}", "-O1", "-Wall", "-Werror=return-type", "-o", exe, SRC,
                           "-L", sc.NATIVE_DIR, "-lsea_current_hip", f"-Wl,-rpath,{sc.NATIVE_DIR}"])
    return exe


@pytest.mark.parametrize("std", ["c++17", "c++20"])
def test_sectors_program_compiles(tmp_path, std):
    import torch
    exe = _build(tmp_path, std)
    if not torch.cuda.is_available():        # without a GPU the program must say so and fail
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode != 0
        assert "no CPU fallback" in r.stderr


@pytest.mark.gpu
def test_sectors_program_on_gpu(tmp_path):
    exe = _build(tmp_path, "c++20")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sectors OK" in r.stdout
