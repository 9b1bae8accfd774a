"""What the CPU tests of the fp64 entries (tests/test_f64_*_abi.py) share: the public header on one line, and a C++ caller of
include/tsqr/blockqr.hpp compiled and linked against the built library."""
import contextlib
import os
import re
import subprocess
import tempfile

from tsqr_gpu_amd import blockqr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_flat():
    """include/tsqr_mi.h on one line: the ' * ' in front of a comment's continuation lines taken out, every run of white space one blank"""
    text = open(os.path.join(ROOT, "include", "tsqr_mi.h")).read()
    return re.sub(r"\s+", " ", re.sub(r"\n \* ", "\n", text))


@contextlib.contextmanager
def compile_and_link(source, name):
    """Build the program `name` in a temporary directory with hipcc against libtsqr_mi.so and yield its path (the directory goes when
    the block ends).  source: C++ text, written to name.cpp there, or the path of a committed .cpp file, compiled where it lies.  A
    failing compile or link raises CalledProcessError."""
    lib_dir = os.path.dirname(blockqr.LIB_PATH)
    with tempfile.TemporaryDirectory() as td:
        src = source
        if not os.path.isfile(source):
            src = os.path.join(td, name + ".cpp")
            with open(src, "w") as f:
                f.write(source)
        exe = os.path.join(td, name)
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-x", "hip", "--offload-arch=gfx950",
                               "-I" + os.path.join(ROOT, "include"), "-o", exe, src,
                               "-L" + lib_dir, "-ltsqr_mi", "-Wl,-rpath," + lib_dir])
        yield exe
