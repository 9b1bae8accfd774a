"""CPU tests of the ordering rule of the stream schedules (tsqr_gpu_amd/csrc/stream_order.h): which neighbouring calls of a batch may
have call i + 1's speculative attempt enqueued before call i is finished.  Too strict a rule silently costs batches their fast schedule;
too loose a rule silently returns wrong factors -- and only the second shows on the GPU (tests/test_gpu_stream_overlap.py).  The header
is plain C++17: a small driver compiled with the host compiler calls it on made-up addresses (nothing is dereferenced)."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
#include "stream_order.h"
using namespace tsqr_order;
static Operands ops(std::uintptr_t q, std::size_t ldq, std::uintptr_t r, std::size_t ldr, std::uintptr_t a, std::size_t lda, std::size_t m, std::size_t n) {
	return operands(reinterpret_cast<const void*>(q), ldq, reinterpret_cast<const void*>(r), ldr, reinterpret_cast<const void*>(a), lda, m, n, 4);
}
extern "C" int pair_conflict(std::uintptr_t q0, std::uintptr_t r0, std::uintptr_t a0, std::uintptr_t q1, std::uintptr_t r1, std::uintptr_t a1,
                             std::size_t ldq, std::size_t ldr, std::size_t lda, std::size_t m, std::size_t n) {
	return conflict(ops(q0, ldq, r0, ldr, a0, lda, m, n), ops(q1, ldq, r1, ldr, a1, lda, m, n)) ? 1 : 0;
}
extern "C" int feeds_itself(std::uintptr_t q, std::uintptr_t r, std::uintptr_t a, std::size_t ldq, std::size_t ldr, std::size_t lda, std::size_t m, std::size_t n) {
	const Operands o = ops(q, ldq, r, ldr, a, lda, m, n);
	return feeds(o, o) ? 1 : 0;
}
"""

M, N, LD = 100, 8, 100
QB = ((N - 1) * LD + M) * 4                             # bytes of a Q or an A operand
RB = ((N - 1) * N + N) * 4                              # bytes of an R operand
BASE = 1 << 32


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("stream_order")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    so = d / "libdriver.so"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", os.path.join(ROOT, "tsqr_gpu_amd", "csrc"),
                           str(src), "-o", str(so)])
    L = ctypes.CDLL(str(so))
    u, s = ctypes.c_uint64, ctypes.c_size_t
    L.pair_conflict.argtypes = [u] * 6 + [s] * 5
    L.feeds_itself.argtypes = [u] * 3 + [s] * 5
    return L


def slots():
    """six well separated operand addresses"""
    return [BASE + k * 4 * QB for k in range(6)]


def conflict(L, q0, r0, a0, q1, r1, a1, ldq=LD, ldr=N, lda=LD, m=M, n=N):
    return L.pair_conflict(q0, r0, a0, q1, r1, a1, ldq, ldr, lda, m, n) == 1


def test_disjoint_operands_do_not_conflict(rule):
    q0, r0, a0, q1, r1, a1 = slots()
    assert not conflict(rule, q0, r0, a0, q1, r1, a1)


def test_exactly_adjacent_ranges_do_not_conflict(rule):
    q0, r0, a0, q1, r1, a1 = slots()
    assert not conflict(rule, q0, r0, a0, q1, r1, q0 + QB)          # A(i + 1) starts where Q(i) ends
    assert not conflict(rule, q0, r0, a0, q1, r1, q0 - QB)          # A(i + 1) ends where Q(i) starts
    assert not conflict(rule, q0, r0, a0, q1, r1, r0 + RB)          # ... where R(i) ends
    assert not conflict(rule, q0, r0, a0, a0 + QB, r1, a1)          # Q(i + 1) right behind A(i)
    assert not conflict(rule, q0, r0, a0, q1, a0 - RB, a1)          # R(i + 1) right in front of A(i)


def test_one_element_of_overlap_at_either_end_conflicts(rule):
    q0, r0, a0, q1, r1, a1 = slots()
    assert conflict(rule, q0, r0, a0, q1, r1, q0 + QB - 4)          # the last element of Q(i) is the first of A(i + 1)
    assert conflict(rule, q0, r0, a0, q1, r1, q0 - QB + 4)          # the first element of Q(i) is the last of A(i + 1)
    assert conflict(rule, q0, r0, a0, q1, r1, r0 + RB - 4)
    assert conflict(rule, q0, r0, a0, q1, r1, r0 - QB + 4)
    assert conflict(rule, q0, r0, a0, a0 + QB - 4, r1, a1)
    assert conflict(rule, q0, r0, a0, q1, a0 - RB + 4, a1)


def test_r_inside_a(rule):
    q0, r0, a0, q1, r1, a1 = slots()
    assert conflict(rule, q0, a1 + 4 * M + 12, a0, q1, r1, a1)      # R(i) in the second column of A(i + 1)
    assert conflict(rule, q0, r0, a0, q1, a0 + 4 * M, a1)           # R(i + 1) inside A(i)


def test_operand_in_the_padding_rows_conflicts(rule):
    """ld > rows: an R placed in the padding rows of A's first column touches no element of A, but the rule compares whole byte ranges
    -- conservative, never too loose"""
    m, n, lda = 100, 2, 128
    rb = ((n - 1) * n + n) * 4
    q0, r0, a0, q1, r1, a1 = slots()
    pad = a1 + 4 * m                                                # rows m .. lda - 1 of column 0
    assert pad + rb <= a1 + 4 * lda
    assert conflict(rule, q0, pad, a0, q1, r1, a1, ldq=m, ldr=n, lda=lda, m=m, n=n)


def test_each_direction(rule):
    q0, r0, a0, q1, r1, a1 = slots()
    # forward: an output of call i is the input of call i + 1
    assert conflict(rule, q0, r0, a0, q1, r1, q0)
    assert conflict(rule, q0, r0, a0, q1, r1, r0)
    # shared outputs: call i's ladder would write after call i + 1
    assert conflict(rule, q0, r0, a0, q0, r1, a1)
    assert conflict(rule, q0, r0, a0, q1, r0, a1)
    assert conflict(rule, q0, r0, a0, r0, r1, a1)                   # Q(i + 1) over R(i)
    assert conflict(rule, q0, r0, a0, q1, q0, a1)                   # R(i + 1) over Q(i)
    # backward: call i + 1 writes over the input of call i
    assert conflict(rule, q0, r0, a0, a0, r1, a1)
    assert conflict(rule, q0, r0, a0, q1, a0, a1)


def test_in_place_calls_do_not_conflict(rule):
    q0, r0, a0, q1, r1, a1 = slots()
    assert not conflict(rule, a0, r0, a0, a1, r1, a1)               # q[i] == a[i] for both calls
    assert rule.feeds_itself(a0, r0, a0, LD, N, LD, M, N) == 1      # ... but a loop over that ONE triple feeds itself
    assert rule.feeds_itself(q0, r0, a0, LD, N, LD, M, N) == 0
    assert rule.feeds_itself(q0, a0 + 8, a0, LD, N, LD, M, N) == 1


def test_the_same_a_read_twice_does_not_conflict(rule):
    q0, r0, a0, q1, r1, a1 = slots()
    assert not conflict(rule, q0, r0, a0, q1, r1, a0)
