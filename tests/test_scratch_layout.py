"""The host helpers of csrc/zmi_scratch.h, checked alone: tests/c/scratch_selftest.cpp includes nothing but that header and is built
here with the address and undefined-behaviour sanitizers (a stand-alone program: nothing sanitized is loaded into this process).  It
checks the carver's two passes, alignment, disjointness and bounds, and the launch-group planner against the formula written out
independently.  The emulator suites (tests/test_emu_*.py) run every entry point with the carver's bound assertion armed.

The textual checks hold zmi_api.hip to stating the launch-group plan and the shared argument checks once."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zlib_rs_amd", "csrc")


def test_carver_and_planner_standalone_under_sanitizers(tmp_path):
    exe = str(tmp_path / "scratch_selftest")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "c", "scratch_selftest.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "scratch_selftest: ok" in r.stdout


def test_scratch_header_is_plain_cxx(tmp_path):
    """no HIP type, nothing of the project: the header compiles as the only include of a translation unit"""
    src = tmp_path / "only.cpp"
    src.write_text('#include "zmi_scratch.h"\nint main() { return (int)zmi_plan_groups(1u << 20, 0, 1, 64, 64).group == 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", CSRC, str(src)], check=True)


def test_api_states_the_plan_and_the_checks_once():
    with open(os.path.join(CSRC, "zmi_api.hip")) as f:
        api = f.read()
    assert api.count('zmi_tune("ZMI_STREAM_GROUP")') == 1
    assert len(re.findall(r"match_per\s*=", api)) <= 1 and api.count("match_per / 16u") <= 1
    assert api.count('"out_align must be a power of two, 1 .. 4096"') == 1
    assert api.count("out_align must be a power of two") == 2          # ... and zmi_tiff_wplan's own text
    assert api.count('"piece_bytes must be 1 .. 2^30"') == 1
    assert api.count('"d_out_len, d_status and d_detail are required"') == 1
    assert "tab_bytes =" not in api and "zmi_bgzf_check_args" not in api
