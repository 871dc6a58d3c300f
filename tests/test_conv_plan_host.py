"""No GPU: the planners of the persistent convolution kernels (csrc/rtn_conv_persistent.h) as a program of their own.

tools/conv_plan_check.cpp includes that header alone - it holds no HIP - and sweeps *_takes / *_choose of generations 4, 5 and 6 over
the Engine's layer shapes, batches, canvases, CU counts, knob values and workspace capacities, asserting for every layer a planner
takes: 1 <= grid <= work items, workspace_bytes <= capacity, K slices that divide the (kernel row, chunk) groups, a stream-K grid
within min(CUs, 8 tiles, tiles x K steps, 1023), and that the choice made with exactly the bytes the sizing call asked for is the
sizing call's choice.  Its header has the -fsanitize command line; here it is built without a sanitizer."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "retinanet-for-table-detection_amd", "csrc")


def test_stand_alone_plan_check_program(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler"
    exe = tmp_path / "conv_plan_check"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                           os.path.join(ROOT, "tools", "conv_plan_check.cpp"), "-o", str(exe)])
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-3000:], run.stderr[-3000:])
    last = run.stdout.splitlines()[-1]
    assert last.startswith("conv plan check:") and last.endswith("0 violations"), last


def test_the_generation_files_know_no_query_mode_and_read_no_knob():
    """What the split is for: a workspace query and a launch run the same planners, and conv_try_persistent (rtn_conv.hip) is the one
    place that reads the knobs and tells the two apart."""
    for name in ("rtn_conv_halo8.hip", "rtn_conv_gemm8.hip", "rtn_conv_halon.hip"):
        with open(os.path.join(CSRC, name)) as f:
            text = f.read()
        assert "query" not in text and "rtn_env_int" not in text, name
    with open(os.path.join(CSRC, "rtn_conv_persistent.h")) as f:
        text = f.read()
    assert "#include <hip" not in text and "rtn_internal.h" not in text and "getenv" not in text and "rtn_env_int" not in text
