"""occupancy_grid::cost_fields_update through the C++ successor header (tests/cpp/test_field_update.cpp): the program
compiles as C++17 and C++20 and fails loudly without a GPU; on the GPU, on a two-room world whose door closes and opens
again, the repaired fields equal cost_fields of the new grid, plain and with the soft knobs on, and it prints OK."""
import os
import subprocess

import pytest

import sea_current_amd as sc

SRC = os.path.join(sc.REPO_ROOT, "tests", "cpp", "test_field_update.cpp")


def _build(tmp_path, std):
    sc.build()
    exe = str(tmp_path / f"test_field_update_{std}")
    subprocess.check_call(["g++", f"-std={std}", "-O1", "-Wall", "-Werror=return-type", "-o", exe, SRC,
                           "-L", sc.NATIVE_DIR, "-lsea_current_hip", f"-Wl,-rpath,{sc.NATIVE_DIR}"])
    return exe


@pytest.mark.parametrize("std", ["c++17", "c++20"])
def test_field_update_program_compiles_and_fails_loudly_without_gpu(tmp_path, std):
    import torch
    exe = _build(tmp_path, std)
    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by the gpu test")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode != 0
    assert "no CPU fallback" in r.stderr


@pytest.mark.gpu
def test_field_update_program_on_gpu(tmp_path):
    exe = _build(tmp_path, "c++20")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "field update OK" in r.stdout
