"""csrc/workspace.h (carve() and the grid / SOR-statistics workspaces cut with it) on the CPU.  A stand-alone host
program (tests/workspace_check.cpp, built here with the system compiler under ASan + UBSan around the header the library
includes) lays every description out into an allocation of exactly the bytes it asks for, writes every element of every
array and checks that the arrays are pairwise disjoint, start on their alignment and end within those bytes; n = 0, 1,
255, 256, 257, a zero-count array in the middle, and a size-only pass at n = 0x7FFFFFFF (the largest n the entry points
accept) against 32-bit overflow.  This file recomputes every byte count with Python's integers."""
import os
import shutil
import subprocess

import pytest

from conftest import PKG, ROOT

ALIGN = 256
BIG = 0x7FFFFFFF


def carve(*sizes):
    """the bytes carve() asks for arrays of these byte sizes: each array starts on ALIGN; never zero"""
    end = 0
    for s in sizes:
        end = (end + ALIGN - 1) // ALIGN * ALIGN + s
    return end or ALIGN


def grid_points(n):  # err, kin, kout, vin, vout, heads, pcell, sxyz
    return carve(4, 8 * n, 8 * n, 4 * n, 4 * n, 4 * n, 4 * n, 24 * n)


def grid_cells(cap, ncells, w3, w5):  # hkeys, hval, nbr3, nbr5, crange, cz
    return carve(8 * cap, 8 * cap, 8 * 9 * ncells * w3, 8 * 25 * ncells * w5, 8 * ncells, 4 * ncells)


def sor_stats(n, F, nvb, aux, job):  # x, sums, vpart, aux, jobs
    return carve(8 * n, 8 * F, 4 * F * nvb, aux, F * job)


def hash_cap(ncells):
    cap = 1
    while cap < 2 * ncells + 2:
        cap <<= 1
    return cap


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path_factory.mktemp("workspace") / "workspace_check"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(ROOT, PKG, "csrc"), os.path.join(ROOT, "tests", "workspace_check.cpp"),
                    "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)  # an ordinary child process
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    lines = [line.split() for line in run.stdout.split("\n") if line.strip()]
    assert lines[-1] == ["OK"]
    return [(line[0], [int(x) for x in line[1:]]) for line in lines[:-1]]


def rows(report, name):
    return [v for k, v in report if k == name]


def test_layouts_disjoint_aligned_in_bounds(report):
    """the program's own checks passed (exit status, above) and covered every n of the grid build and the statistics"""
    for name in ("grid_points", "grid_cells", "sor_stats"):
        assert {v[1] if name == "grid_cells" else v[0] for v in rows(report, name)} == {0, 1, 255, 256, 257}
    cells = rows(report, "grid_cells")
    assert {(v[2], v[3]) for v in cells} == {(0, 0), (1, 0), (0, 1), (1, 1)}  # zero-count arrays in the middle
    assert {v[1] for v in rows(report, "sor_stats")} == {1, 3}


def test_bytes_match_python(report):
    for n, b in rows(report, "grid_points"):
        assert b == grid_points(n)
    for cap, ncells, w3, w5, b in rows(report, "grid_cells"):
        assert cap == hash_cap(ncells) and b == grid_cells(cap, ncells, w3, w5)
    for n, F, nvb, aux, job, b in rows(report, "sor_stats"):
        assert b == sor_stats(n, F, nvb, aux, job)
    assert rows(report, "plain") == [[carve(20, 0, 3, 8 * 33)]]
    assert rows(report, "empty") == [[carve(0)]] == [[ALIGN]]


def test_no_32_bit_overflow_at_the_largest_n(report):
    (n, b), = rows(report, "big_grid_points")
    assert n == BIG and b == grid_points(BIG) and b > 56 * BIG
    (cap, ncells, w3, w5, b), = rows(report, "big_grid_cells")
    assert ncells == BIG and cap == hash_cap(BIG) == 1 << 32 and b == grid_cells(cap, BIG, w3, w5) and b > 1 << 38
    (n, F, nvb, aux, job, b), = rows(report, "big_sor_stats")
    assert n == BIG and b == sor_stats(n, F, nvb, aux, job) and b > 8 * BIG
