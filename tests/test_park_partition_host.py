"""The parked fold's split of a model among its workgroups (fedn_amd/csrc/park_partition.h, the one
definition the kernel fedavg_park_body and its launcher share), compiled for the CPU.

A model of P elements is whole tall tiles (HEIGHT consecutive small tiles each, dealt to the grid's
workgroups wg, wg + G, ... through the load ring), up to HEIGHT - 1 leftover whole small tiles and at
most one ragged tile (each through k_fedavg_tail, in the workgroup the header names). Every element
must belong to exactly one of these, and their union must be [0, P): for every P from 0 to three tall
tiles + 1 (element by element, on a small tile so that this stays quick), and for a few thousand
random larger P at the kernel's 4096-element tile (by intervals), HEIGHT 1, 2, 4, grids of 1, 2, 3, 256.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEIGHTS = (1, 2, 4)
GRIDS = (1, 2, 3, 256)

# stdin: lines "P tile height grid"; stdout per line: ntall nleft ragged, then every workgroup's
# ring-tile count, then every tail tile's owner
PROG = r"""
#include <cinttypes>
#include <cstdio>
#include "park_partition.h"
int main() {
    long long P, tile, height, grid;
    while (std::scanf("%lld %lld %lld %lld", &P, &tile, &height, &grid) == 4) {
        const ParkPartition p = park_partition(P, tile, (int)height);
        std::printf("%" PRId64 " %d %d", p.ntall, p.nleft, p.ragged);
        for (long long wg = 0; wg < grid; ++wg) std::printf(" %" PRId64, park_ring_tiles(p, grid, wg));
        for (int j = 0; j < p.ntail(); ++j) std::printf(" %" PRId64, park_tail_owner(p, grid, j));
        std::printf(" %" PRId64 "\n", p.units());
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def part_exe(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "a C++ compiler is needed (build() needs one too)"
    d = tmp_path_factory.mktemp("parkpart")
    src = d / "part.cpp"
    src.write_text(PROG)
    exe = d / "part"
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "fedn_amd", "csrc"), str(src),
                    "-o", str(exe)], check=True)
    return exe


def _ask(exe, queries):
    """[(P, tile, height, grid)] -> [(ntall, nleft, ragged, ring counts, tail owners)]"""
    text = "".join("%d %d %d %d\n" % q for q in queries)
    lines = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(lines) == len(queries)
    out = []
    for (P, tile, height, grid), line in zip(queries, lines):
        v = [int(x) for x in line.split()]
        ntall, nleft, ragged = v[:3]
        ntail = nleft + (1 if ragged else 0)
        assert len(v) == 3 + grid + ntail + 1, line
        assert v[-1] == ntall + ntail, "units(): what the launcher sizes the grid by"
        out.append((ntall, nleft, ragged, v[3:3 + grid], v[3 + grid:-1]))
    return out


def _pieces(P, tile, height, grid, ans):
    """Every (owner, start, stop) the kernel would fold, as it derives them from the partition: ring
    tile i of workgroup wg is tall tile wg + i * grid; tail tile j is small tile ntall * height + j,
    clipped at P (k_fedavg_tail stops there)."""
    ntall, nleft, ragged, ring, owners = ans
    tall = tile * height
    out = []
    for wg, cnt in enumerate(ring):
        for i in range(cnt):
            t = wg + i * grid
            out.append((wg, t * tall, (t + 1) * tall))
    for j, wg in enumerate(owners):
        start = (ntall * height + j) * tile
        out.append((wg, start, min(start + tile, P)))
    return out


def _check_shape(P, tile, height, grid, ans):
    ntall, nleft, ragged, ring, owners = ans
    what = f"P={P} tile={tile} height={height} grid={grid}"
    assert 0 <= nleft < height and 0 <= ragged < tile, what
    assert (ntall * height + nleft) * tile + ragged == P, what
    assert all(0 <= wg < grid for wg in owners), what
    if len(owners) <= grid:
        assert len(set(owners)) == len(owners), what + ": tail tiles share a workgroup though the grid has enough"
    return what


@pytest.mark.parametrize("height", HEIGHTS)
def test_every_element_once_small_models(part_exe, height):
    """P = 0 .. 3 tall tiles + 1, element by element (a tile of 8 elements: the function knows no other
    constant of the kernel)."""
    tile = 8
    queries = [(P, tile, height, grid) for grid in GRIDS for P in range(3 * height * tile + 2)]
    for q, ans in zip(queries, _ask(part_exe, queries)):
        P, _, _, grid = q
        what = _check_shape(*q, ans)
        seen = np.zeros(P, dtype=np.int32)
        for wg, a, b in _pieces(*q, ans):
            assert 0 <= a < b <= P, what                      # nothing empty, nothing outside the model
            seen[a:b] += 1
        assert (seen == 1).all(), what


@pytest.mark.parametrize("height", HEIGHTS)
def test_every_element_once_large_models(part_exe, height):
    """A few thousand random larger P at the kernel's tile, by intervals: sorted, the pieces must
    tile [0, P) with no gap and no overlap. The sizes keep a workgroup's ring list short enough to
    enumerate (up to 400 tall tiles), with a few at the workload's scale and beyond 2^31 elements
    checked through the counts alone."""
    tile = 4096
    rng = np.random.default_rng(20260521 + height)
    Ps = [int(p) for p in rng.integers(3 * height * tile + 2, 400 * height * tile, 1000)]
    queries = [(P, tile, height, grid) for grid in GRIDS for P in Ps]
    for q, ans in zip(queries, _ask(part_exe, queries)):
        P = q[0]
        what = _check_shape(*q, ans)
        pieces = sorted((a, b) for _, a, b in _pieces(*q, ans))
        at = 0
        for a, b in pieces:
            assert a == at and b > a, what
            at = b
        assert at == P, what
    huge = [100_000_000, (1 << 31) + 5, (1 << 33) + 4096 * height - 1, (1 << 40) + 12345]
    queries = [(P, tile, height, grid) for grid in GRIDS for P in huge]
    for q, ans in zip(queries, _ask(part_exe, queries)):
        P, _, _, grid = q
        what = _check_shape(*q, ans)
        ntall, ring = ans[0], ans[3]
        # workgroup wg's tiles are wg, wg + grid, ... < ntall: exactly the residues, so the counts decide
        assert ring == [len(range(wg, ntall, grid)) for wg in range(grid)], what
