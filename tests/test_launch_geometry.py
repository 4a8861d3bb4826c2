"""voltrix/launch_geometry.hpp is host code that compiles without HIP, and its two grids are the formulas every launch_* function
carried before they were shared -- restated here in Python, compared on every input of a fixed list through a small program with its
own ``main``.  No GPU, nothing loaded into Python."""
import itertools
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(REPO, "voltrix-spmm_amd", "voltrix", "include")
NUM_XCD, CHUNK_EDGES = 8, 128

PIECES = (1, 2, 3, 4, 5, 63, 64, 65, 128, 129)
HEADS = (1, 2, 3, 8, 64, 65, 65535, 65536)
NUM_ROWS = (1, 255, 256, 257, 2 ** 31 - 1)
NNZ = (1, 127, 128, 129, 2 ** 31 - 1)
# beyond the list above, which reaches the slab limit only through heads = 65536: the first width past 65535 slabs of 64 pieces, and
# an edge count whose workgroups no longer fit a grid (the launchers refuse nnz > INT_MAX earlier; the helper takes 64 bits)
ROW_CASES = list(itertools.product(NUM_ROWS, PIECES)) + [(1, 65535 * 64), (1, 65535 * 64 + 1)]
EDGE_CASES = list(itertools.product(NNZ, HEADS, PIECES)) + [(2 ** 40, 1, 64), (2 ** 40, 65536, 64), (2 ** 36, 8, 1)]

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <type_traits>

#include "voltrix/launch_geometry.hpp"

int main(int argc, char** argv) {
  using namespace voltrix;
  for (int i = 1; i + 1 < argc;) {
    if (argv[i][0] == 'r') {
      const RowGroupGrid g = row_group_grid(std::atoi(argv[i + 1]), std::atoi(argv[i + 2]));
      std::printf("r %d %d %d %lld %d\n", g.lanes, g.slabs, g.rows_per_group, g.per_xcd, (int)g.ok);
      i += 3;
    } else {
      const EdgeChunkGrid g = edge_chunk_grid(std::atoll(argv[i + 1]), std::atoi(argv[i + 2]), std::atoi(argv[i + 3]), 128);
      std::printf("e %d %d %d %d %d %d %lld %lld %d\n", g.head_lanes, g.head_shift, g.rounds, g.slab_heads, g.lanes, g.slabs, g.wgs,
                  g.per_xcd, (int)g.ok);
      i += 4;
    }
  }
  // the small helpers
  alignas(16) static char buf[32];
  int sizes = 0;
  long long pairs = 0;
  for (int d = 0; d < 3; ++d) dispatch_feature_type(d, [&](auto tag) { sizes = sizes * 10 + (int)sizeof(tag); });
  for (int x = 0; x < 3; ++x)
    for (int y = 0; y < 3; ++y)
      if (sddmm_pair_ok(x, y)) dispatch_sddmm_pair(x, y, [&](auto xt, auto yt) { pairs = pairs * 100 + 10 * (int)sizeof(xt) + (int)sizeof(yt); });
  std::printf("h %d %d %d %d %d %d %d %d %d %d\n", piece_elems(0), piece_elems(1), piece_elems(2), (int)bad_ptr(nullptr, 15),
              (int)bad_ptr(buf, 15), (int)bad_ptr(buf + 4, 15), (int)bad_ptr(buf + 4, 3), (int)misaligned(nullptr, 15),
              (int)misaligned(buf + 2, 3), (int)misaligned(buf + 16, 15));
  std::printf("d %d %lld\n", sizes, pairs);
  return 0;
}
"""


def row_group_grid(num_rows, pieces):
    """launch_spmm_csr_heads / attn_aggregate (forward, d_feat) / gatv2_rowsum before the header existed."""
    slab_pieces = min(pieces, 64)
    lanes = 1
    while lanes < slab_pieces:
        lanes <<= 1
    slabs = (pieces + 63) // 64
    rows_per_group = 256 // lanes
    groups = (num_rows + rows_per_group - 1) // rows_per_group
    per_xcd = (groups + NUM_XCD - 1) // NUM_XCD
    bad = per_xcd * NUM_XCD > 0x7FFFFFFF or slabs > 65535
    return (lanes, slabs, rows_per_group, per_xcd, int(not bad)), (per_xcd * NUM_XCD > 0x7FFFFFFF, slabs > 65535)


def edge_chunk_grid(nnz, heads, pieces):
    """launch_sddmm_heads_csr / gatv2_score / attn_aggregate d_s before the header existed."""
    head_lanes, head_shift = 1, 0
    while head_lanes < pieces and head_lanes < 64:
        head_lanes <<= 1
        head_shift += 1
    rounds = (pieces + head_lanes - 1) // head_lanes
    slab_heads = min(heads, 64 // head_lanes)
    lanes = head_lanes
    while lanes < slab_heads * head_lanes:
        lanes <<= 1
    slabs = (heads + slab_heads - 1) // slab_heads
    chunks = (nnz + CHUNK_EDGES - 1) // CHUNK_EDGES
    groups_per_wg = 256 // lanes
    wgs = (chunks + groups_per_wg - 1) // groups_per_wg
    per_xcd = (wgs + NUM_XCD - 1) // NUM_XCD
    bad = per_xcd * NUM_XCD > 0x7FFFFFFF or slabs > 65535
    return ((head_lanes, head_shift, rounds, slab_heads, lanes, slabs, wgs, per_xcd, int(not bad)),
            (per_xcd * NUM_XCD > 0x7FFFFFFF, slabs > 65535))


def single_head_grid(nnz, pieces):
    """launch_sddmm_csr before the header existed: one head, no slab limit -> (lanes, rounds, wgs, per_xcd, ok)."""
    lanes = 1
    while lanes < min(pieces, 64):
        lanes <<= 1
    rounds = (pieces + lanes - 1) // lanes
    chunks = (nnz + CHUNK_EDGES - 1) // CHUNK_EDGES
    groups_per_wg = 256 // lanes
    wgs = (chunks + groups_per_wg - 1) // groups_per_wg
    per_xcd = (wgs + NUM_XCD - 1) // NUM_XCD
    return lanes, rounds, wgs, per_xcd, int(not per_xcd * NUM_XCD > 0x7FFFFFFF)


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    work = tmp_path_factory.mktemp("launch_geometry")
    src, exe = work / "main.cpp", work / "main"
    src.write_text(PROGRAM)
    # -x c++: a plain host compile, no HIP header, no device pass; the sanitizers are the host's and check the stand-alone program
    subprocess.check_call([hipcc, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-Xarch_host", "-fsanitize=address",
                           "-Xarch_host", "-fsanitize=undefined", "-fno-sanitize-recover=all", f"-I{INCLUDE}", str(src), "-o", str(exe)])
    args = []
    for num_rows, pieces in ROW_CASES:
        args += ["r", str(num_rows), str(pieces)]
    for nnz, heads, pieces in EDGE_CASES:
        args += ["e", str(nnz), str(heads), str(pieces)]
    out = subprocess.run([str(exe)] + args, check=True, capture_output=True, text=True).stdout.splitlines()
    return [line.split() for line in out]


def test_header_has_no_device_code():
    with open(os.path.join(INCLUDE, "voltrix", "launch_geometry.hpp")) as f:
        text = f.read()
    for word in ("__device__", "__global__", "hip_runtime", "hipLaunch", "dim3"):
        assert word not in text.split("#pragma once")[1], word


def test_row_group_grid_is_the_parents_formula(printed):
    rows = [line for line in printed if line[0] == "r"]
    assert len(rows) == len(ROW_CASES)
    limits = [False, False]
    for (num_rows, pieces), line in zip(ROW_CASES, rows):
        want, hit = row_group_grid(num_rows, pieces)
        assert tuple(int(v) for v in line[1:]) == want, (num_rows, pieces)
        limits = [a or b for a, b in zip(limits, hit)]
    # an int row count over at least 4 rows per group cannot overflow grid.x: only the slab limit is reachable here
    assert limits == [False, True]


def test_edge_chunk_grid_is_the_parents_formula(printed):
    rows = [line for line in printed if line[0] == "e"]
    assert len(rows) == len(EDGE_CASES)
    limits = [False, False]
    for (nnz, heads, pieces), line in zip(EDGE_CASES, rows):
        want, hit = edge_chunk_grid(nnz, heads, pieces)
        assert tuple(int(v) for v in line[1:]) == want, (nnz, heads, pieces)
        limits = [a or b for a, b in zip(limits, hit)]
        if heads == 1:       # launch_sddmm_csr reads lanes, rounds, wgs, per_xcd and ok of the one-head grid
            got = tuple(int(line[i]) for i in (5, 3, 7, 8, 9))
            assert got == single_head_grid(nnz, pieces), (nnz, pieces)
    assert limits == [True, True]       # refusals from both limits: grid.x past 2^31 - 1, more than 65535 slabs


def test_small_helpers(printed):
    helpers = next(line for line in printed if line[0] == "h")
    #                      piece_elems   bad_ptr: null, aligned, +4 & 15, +4 & 3   misaligned: null, +2 & 3, +16 & 15
    assert helpers[1:] == ["4", "8", "8", "1", "0", "1", "0", "0", "1", "0"]
    dispatch = next(line for line in printed if line[0] == "d")
    # float, _Float16, 16-bit storage; the five pairs in (x, y) order: (4,4) (4,2) (4,2) (2,2) (2,2)
    assert dispatch[1:] == ["422", "4442422222"]
