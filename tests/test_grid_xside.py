"""csrc/grid_xside.hpp compiled for the host: the shared hash-grid cell arithmetic -- cell and fraction, the row index forms, the weights, the x-side
row helper of the lane-pair lookup -- against plain restatements of the reference's per-corner index and weight loop
(tests/native/grid_xside_check.cpp)."""
import os
import subprocess


def test_x_side_rows_equal_the_eight_corner_form(tmp_path):
    """Random cells, resolutions and table sizes -- powers of two and not, dense and hashed levels, sizes right at the dense / hashed switch, tiled grids,
    the far-face cells -- for D = 2 and D = 3 with align_corners both ways, through the form level_kind() picks and through the general form; grid_cell at
    0, 1, the largest float below 1 and on cell borders; the weights in the reference's order of multiplications.  A stand-alone program under the
    address and undefined-behaviour sanitizers (its own process, nothing preloaded).  Exit status 0 = every case agrees."""
    exe = tmp_path / "grid_xside_check"
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "grid_xside_check.cpp")
    subprocess.check_call(["g++", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover", "-o", str(exe), src])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
