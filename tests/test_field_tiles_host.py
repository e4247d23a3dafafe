"""csrc/frame_plan.hpp compiled for the host: field_wave_tile, the static deal of wave tiles to the waves of the NeRF field launch
(tests/native/field_tiles_check.cpp)."""
import os
import subprocess


def test_field_wave_tiles_are_dealt_exactly_once(tmp_path):
    """Grids of 1, 2, 511 and 512 workgroups of 8 waves, tile counts from 0 past three full rounds: every wave tile comes up exactly once, a wave's
    tiles ascend until its first one out of range, and no two waves' loads differ by more than one; a stand-alone program under the address and
    undefined-behaviour sanitizers (its own process, nothing preloaded).  Exit status 0 = every case holds."""
    exe = tmp_path / "field_tiles_check"
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "field_tiles_check.cpp")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover", "-o", str(exe), src])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
