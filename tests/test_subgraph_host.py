"""CPU: the induced-subgraph contract, the walk rule and their plumbing.  The numpy restatement
(tests/subgraph_oracle.py) reproduces the known answers of the walk rule, walks uniformly and restricts a hand-written CSR to the
arrays written out here; a stand-alone host program runs the header's own ``walk_one`` / ``walk_step`` -- the code the kernel runs --
and agrees with it; the three entry points are declared, bound and exported; their argument checks are rows of
tests/core_abi_cases.py; the Python layer raises before it looks at a tensor; every kernel, in every lane-group width, compiles for
gfx950 without scratch and without spilled registers.  No GPU compute is called here (tests/test_gpu_subgraph.py compares the kernels with the same
oracle)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO

import subgraph_oracle as oracle
from kernel_resources import resource_usage
from voltrix import capi

HEADER = os.path.join(REPO, "include", "voltrix_capi.h")
INCLUDE = os.path.join(REPO, "voltrix-spmm_amd", "voltrix", "include")
NAMES = ("voltrix_launch_subgraph_count", "voltrix_launch_subgraph_fill", "voltrix_launch_random_walk")
GROUPS = (4, 8, 16, 32, 64)


def _ring():
    """100 nodes, row v = [(v + 1) % 100, (v + 7) % 100, (v + 31) % 100]."""
    n = 100
    return np.arange(0, 3 * n + 1, 3), np.array([[(v + 1) % n, (v + 7) % n, (v + 31) % n] for v in range(n)]).ravel()


def _dead_ends():
    """50 rows: degree v % 4 (every fourth node is a dead end), and one column outside [0, 50), which ends a walk as well."""
    n = 50
    degrees = np.arange(n) % 4
    indptr = np.concatenate([[0], np.cumsum(degrees)])
    indices = np.concatenate([(v * 7 + np.arange(d) * 13 + 1) % n for v, d in enumerate(degrees)])
    indices[indptr[7]] = 60
    return indptr, indices


# ---- the walk rule
def test_known_answers_of_the_walk_rule():
    indptr, indices = _ring()
    nodes, entries = oracle.random_walk(indptr, indices, [0, 0, 5, 99], 9, 9, 0)
    assert nodes[0].tolist() == [0, 1, 2, 3, 4, 35, 36, 67, 68, 75]
    assert entries[0].tolist() == [0, 3, 6, 9, 14, 105, 110, 201, 205]
    assert nodes[1].tolist() == [0, 31, 32, 39, 70, 77, 84, 91, 22, 29]                 # the same start, another walker: another walk
    assert nodes[3].tolist() == [99, 0, 1, 2, 3, 4, 11, 42, 43, 50]
    assert np.array_equal(indices[entries], nodes[:, 1:])
    high, _ = oracle.random_walk(indptr, indices, [0, 0, 5, 99], 9, 2 ** 40 + 9, 2 ** 32 + 7)     # the high words of seed and offset
    assert high[0].tolist() == [0, 7, 14, 21, 52, 83, 90, 97, 98, 29]
    # the draws carry bits 31 and 30 in counter word 1: neither the dropout mask's nor the neighbour sampler's words
    import sample_oracle
    from test_attn_dropout_host import philox4x32_10

    walkers = np.arange(4)
    mask_words = np.stack(philox4x32_10(walkers, 0, 0, 0, 9, 0), -1)
    assert not (oracle.walk_draws(walkers, 4, 9, 0) == mask_words).any()
    assert not (oracle.walk_draws(walkers, 4, 9, 0) == sample_oracle.draws(walkers, 4, 9, 0)).any()


def test_a_walk_ends_at_a_dead_end_and_at_a_column_out_of_range():
    indptr, indices = _dead_ends()
    nodes, entries = oracle.random_walk(indptr, indices, np.concatenate([np.arange(50), np.full(14, 7)]), 3, 5, 1)
    assert (nodes[:50:4, 1:] == -1).all() and (entries[:50:4] == -1).all()                   # a start of degree 0
    ended = (nodes == -1).any(1)
    assert ended.any() and not ended.all()
    for w in range(64):
        over = np.flatnonzero(nodes[w] == -1)
        if over.size:                                                                    # -1 from the first dead end on, in both
            last = nodes[w, over[0] - 1]
            assert (nodes[w, over[0]:] == -1).all() and (entries[w, over[0] - 1:] == -1).all()
            assert last == 60 or indptr[last + 1] == indptr[last]
    assert (nodes == 60).any()                                                           # recorded as it is, then the walk is over


@pytest.mark.parametrize("degree", [2, 7, 64, 300])
def test_one_step_takes_every_neighbour_equally(degree):
    """40,000 walkers one step from a node of degree d: every neighbour's count within 5 sigma of n / d (binomial sigma).  The
    multiply-shift's bias, at most d / 2^32 relative, is orders of magnitude below one sigma."""
    n = 40000
    indptr = np.concatenate([[0], np.full(degree + 1, degree)])                          # node 0 points at 1 .. d, which are dead ends
    indices = np.arange(1, degree + 1)
    nodes, entries = oracle.random_walk(indptr, indices, np.zeros(n, np.int64), 1, 20261019, 3)
    assert np.array_equal(nodes[:, 1], entries[:, 0] + 1)
    p = 1 / degree
    counts = np.bincount(entries[:, 0], minlength=degree)
    worst = np.abs(counts - n * p).max() / (n * p * (1 - p)) ** 0.5
    print(f"d={degree}: worst deviation {worst:.2f} sigma")
    assert counts.size == degree and worst <= 5, (degree, worst)


def _complete_walks(seed):
    n, k = 40000, 8
    return n, k, oracle.random_walk(np.arange(0, k * k + 1, k), np.tile(np.arange(k), k), np.zeros(n, np.int64), 12, seed, 3)[0]


def test_twelve_steps_on_a_complete_graph_stay_uniform():
    n, k, nodes = _complete_walks(20261019)
    p = 1 / k
    for t in range(1, 13):                                                               # across the Philox blocks at t = 4, 8
        counts = np.bincount(nodes[:, t], minlength=k)
        worst = np.abs(counts - n * p).max() / (n * p * (1 - p)) ** 0.5
        print(f"step {t}: worst deviation {worst:.2f} sigma")
        assert worst <= 5, (t, worst)


def test_consecutive_steps_are_independent():
    n, k, nodes = _complete_walks(1)
    p = 1 / (k * k)
    for t in range(1, 12):
        counts = np.bincount(nodes[:, t] * k + nodes[:, t + 1], minlength=k * k)
        worst = np.abs(counts - n * p).max() / (n * p * (1 - p)) ** 0.5
        print(f"steps {t}, {t + 1}: worst cell deviates {worst:.2f} sigma")
        assert worst <= 5, (t, worst)


# ---- the header's own walk code in a host program
PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "voltrix/induced_subgraph_kernels.hpp"

// argv: graph file (num_rows, indptr, the number of entries, indices), length, seed, offset, starts ...
int main(int argc, char** argv) {
  if (argc < 5) return 2;
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 3;
  int num_rows = 0, count = 0;
  if (std::fscanf(f, "%d", &num_rows) != 1) return 4;
  std::vector<int> indptr(num_rows + 1);
  for (int& v : indptr) if (std::fscanf(f, "%d", &v) != 1) return 4;
  if (std::fscanf(f, "%d", &count) != 1) return 4;
  std::vector<int> indices(count);
  for (int& v : indices) if (std::fscanf(f, "%d", &v) != 1) return 4;
  std::fclose(f);
  const int length = std::atoi(argv[2]);
  const unsigned long long seed = std::strtoull(argv[3], nullptr, 10), offset = std::strtoull(argv[4], nullptr, 10);
  const int walkers = argc - 5;
  // exactly as large as the contract says: the host's sanitizer sees a store outside [W, length + 1] / [W, length]
  std::vector<int> nodes((size_t)walkers * (length + 1), -7), entries((size_t)walkers * length, -7);
  std::vector<int> nodes_t(nodes.size(), -7), entries_t(entries.size(), -7);
  for (int w = 0; w < walkers; ++w) {
    const int start = std::atoi(argv[5 + w]);
    voltrix::walk_one(indptr.data(), indices.data(), num_rows, (uint32_t)w, start, length, (uint32_t)seed, (uint32_t)(seed >> 32),
                      (uint32_t)offset, (uint32_t)(offset >> 32), nodes.data(), length + 1, 1, entries.data(), length, 1);
    voltrix::walk_one(indptr.data(), indices.data(), num_rows, (uint32_t)w, start, length, (uint32_t)seed, (uint32_t)(seed >> 32),
                      (uint32_t)offset, (uint32_t)(offset >> 32), nodes_t.data(), 1, walkers, entries_t.data(), 1, walkers);
  }
  for (int w = 0; w < walkers; ++w) {
    std::printf("n");
    for (int t = 0; t <= length; ++t) {
      if (nodes[(size_t)w * (length + 1) + t] != nodes_t[(size_t)t * walkers + w]) return 5;      // step-major: the same walk
      std::printf(" %d", nodes[(size_t)w * (length + 1) + t]);
    }
    std::printf("\ne");
    for (int t = 0; t < length; ++t) {
      if (entries[(size_t)w * length + t] != entries_t[(size_t)t * walkers + w]) return 5;
      std::printf(" %d", entries[(size_t)w * length + t]);
    }
    std::printf("\n");
  }
  return 0;
}
"""

#       (graph, starts, length, seed, offset)
WALKS = [("ring", [0, 0, 5, 99], 9, 9, 0), ("ring", [0, 0, 5, 99], 9, 2 ** 40 + 9, 2 ** 32 + 7),
         ("ring", list(range(100)), 33, 20261019, 3),
         ("ring", [4], 0, 1, 1), ("ring", [4, 4], 1, 2 ** 64 - 1, 2 ** 64 - 1), ("dead", list(range(50)), 12, 5, 1),
         ("dead", [7] * 40, 5, 2 ** 63 + 1, 2 ** 32 + 5), ("dead", [1, 2, 3], 4, 20261019, 2 ** 32 + 7)]


def test_host_and_device_run_the_same_walk_code(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src, exe = tmp_path / "main.hip", tmp_path / "main"
    src.write_text(PROGRAM)
    # the header as HIP (its kernels are compiled for gfx950 and not launched: the program makes no HIP runtime call); the sanitizers
    # are the host's and check the stand-alone program
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", "-Wall", "-Werror", "-Xarch_host", "-fsanitize=address",
                           "-Xarch_host", "-fsanitize=undefined", "-fno-sanitize-recover=all", f"-I{INCLUDE}", str(src), "-o", str(exe)])
    graphs = {"ring": _ring(), "dead": _dead_ends()}
    for name, (indptr, indices) in graphs.items():
        (tmp_path / name).write_text(" ".join(str(int(v)) for v in [indptr.size - 1, *indptr, indices.size, *indices]))
    for name, starts, length, seed, offset in WALKS:
        run = subprocess.run([str(exe), str(tmp_path / name), str(length), str(seed), str(offset)] + [str(s) for s in starts],
                             check=True, capture_output=True, text=True)
        lines = run.stdout.splitlines()
        assert len(lines) == 2 * len(starts)
        nodes, entries = oracle.random_walk(*graphs[name], starts, length, seed, offset)
        for w in range(len(starts)):
            assert lines[2 * w][0] == "n" and [int(v) for v in lines[2 * w].split()[1:]] == nodes[w].tolist(), (name, seed, w)
            assert lines[2 * w + 1][0] == "e" and [int(v) for v in lines[2 * w + 1].split()[1:]] == entries[w].tolist(), (name, seed, w)


# ---- the subgraph contract
#          r0  r1         r2         r3            r4       r5       r6   r7         r8       r9  r10           r11
HAND = ([], [3, 5, 7], [1, 1, 4], [9, 2, 6, 0], [8, 10], [0, 11], [2], [5, 5, 5], [11, 3], [], [4, 6, 7, 9], [1, 0])


def _hand():
    return np.concatenate([[0], np.cumsum([len(r) for r in HAND])]), np.concatenate([np.array(r, np.int64) for r in HAND])


def test_oracle_restricts_a_hand_written_csr():
    indptr, indices = _hand()
    assert indptr.tolist() == [0, 0, 3, 6, 10, 12, 14, 15, 18, 20, 20, 24, 26]
    # an unsorted row, an empty row, a row with a duplicate column, a row with nothing selected, three times one column, the unsorted
    # row again (a duplicate in `rows`), a sorted row; local ids: 5 -> 0, 1 -> 1, 9 -> 2, 0 -> 3, 6 -> 4
    rows, cols = [3, 0, 2, 4, 7, 3, 10], [5, 1, 9, 0, 6]
    s_indptr, s_local, s_entries = oracle.subgraph_csr(indptr, indices, rows, cols, 12)
    assert s_indptr.tolist() == [0, 3, 3, 5, 5, 8, 11, 13]
    assert s_local.tolist() == [2, 4, 3, 1, 1, 0, 0, 0, 2, 4, 3, 4, 2]                   # CSR order: row 3 stays 9, 6, 0
    assert s_entries.tolist() == [6, 8, 9, 3, 4, 15, 16, 17, 6, 8, 9, 21, 23]
    assert all(a.dtype == np.int32 for a in (s_indptr, s_local, s_entries))
    assert np.array_equal(np.array(cols)[s_local], indices[s_entries])
    # eight columns only: the 9 of row 3 is outside [0, num_cols) and is never selected
    s_indptr, s_local, s_entries = oracle.subgraph_csr(indptr, indices, [3], [5, 1, 0, 6], 8)
    assert (s_indptr.tolist(), s_local.tolist(), s_entries.tolist()) == ([0, 2], [3, 2], [8, 9])
    # cols defaults to rows: the square case
    s_indptr, s_local, s_entries = oracle.subgraph_csr(indptr, indices, [5, 11, 0, 1])
    assert (s_indptr.tolist(), s_local.tolist(), s_entries.tolist()) == ([0, 2, 4, 4, 5], [2, 1, 3, 2, 0], [12, 13, 24, 25, 1])
    sub = oracle.induced_subgraph(indptr, indices, [5, 11, 0, 1])
    assert sub["indices"].tolist() == [2, 1, 3, 2, 0] and sub["node_ids"].tolist() == [5, 11, 0, 1] and sub["num_nodes"] == 4


def test_oracle_identity_returns_the_csr_itself():
    indptr, indices = _hand()
    s_indptr, s_local, s_entries = oracle.subgraph_csr(indptr, indices, np.arange(12))
    assert np.array_equal(s_indptr, indptr) and np.array_equal(s_local, indices) and np.array_equal(s_entries, np.arange(26))
    ring = _ring()
    s_indptr, s_local, s_entries = oracle.subgraph_csr(*ring, np.arange(100), np.arange(100), 100)
    assert np.array_equal(s_indptr, ring[0]) and np.array_equal(s_local, ring[1]) and np.array_equal(s_entries, np.arange(300))
    visited = oracle.sample_subgraph_rw(*ring, [0, 0, 5, 99], 9, 9)
    walked, _ = oracle.random_walk(*ring, [0, 0, 5, 99], 9, 9)
    assert np.array_equal(visited["node_ids"], np.unique(walked)) and (np.diff(visited["node_ids"]) > 0).all()


# ---- plumbing
def test_header_declares_and_binding_lists_the_entry_points():
    import voltrix

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in capi.SYMBOLS and name in capi.SIGNATURES, name
        assert hasattr(capi.lib(), name)
    assert capi.lib().voltrix_abi_version() == 2
    for fn in (voltrix.subgraph_csr, voltrix.induced_subgraph, voltrix.random_walk, voltrix.sample_subgraph_rw):
        assert callable(fn)
    assert voltrix.Subgraph is voltrix.subgraph.Subgraph and capi.SUBGRAPH_GROUPS == GROUPS == voltrix.subgraph.GROUPS
    assert capi.WALK_MAX_LENGTH == voltrix.subgraph.MAX_WALK_LENGTH == 2 ** 20
    for wrapper in ("launch_subgraph_count", "launch_subgraph_fill", "launch_random_walk"):
        assert not hasattr(getattr(capi, wrapper), "timer_label"), wrapper
    assert [voltrix.subgraph.group_for(nnz, 10) for nnz in (0, 40, 41, 80, 160, 320, 321, 10 ** 6)] == [4, 4, 8, 8, 16, 32, 64, 64]


def test_python_layer_rejects_bad_arguments_before_any_tensor_is_looked_at():
    import torch
    import voltrix

    for length in (-1, 2 ** 20 + 1, 2.0, "4", None, True):
        with pytest.raises(ValueError):
            voltrix.random_walk(None, None, None, length, 1)
        with pytest.raises(ValueError):
            voltrix.sample_subgraph_rw(None, None, None, length, 1)
    for seed, offset in ((-1, 0), (2 ** 64, 0), (0, -1), (0, 2 ** 64), (1.5, 0), (0, None)):
        with pytest.raises(ValueError):
            voltrix.random_walk(None, None, None, 4, seed, offset)
        with pytest.raises(ValueError):
            voltrix.sample_subgraph_rw(None, None, None, 4, seed, offset)
    host = torch.zeros(4, dtype=torch.int32)
    wide = torch.zeros(4, dtype=torch.int64)
    for bad in (host, wide, None, [0, 1]):                       # tensors are looked at next: host, int64 or no tensors at all
        with pytest.raises(ValueError):
            voltrix.subgraph_csr(bad, bad, bad)
        with pytest.raises(ValueError):
            voltrix.induced_subgraph(bad, bad, bad)
        with pytest.raises(ValueError):
            voltrix.random_walk(bad, bad, bad, 4, 1)
        with pytest.raises(ValueError):
            voltrix.sample_subgraph_rw(bad, bad, bad, 4, 1)


SOURCE = r'''
#include "voltrix/induced_subgraph_kernels.hpp"
#define BOTH(G) template __global__ void voltrix::subgraph_kernel<G, false>(const voltrix::SubgraphArgs); \
                template __global__ void voltrix::subgraph_kernel<G, true>(const voltrix::SubgraphArgs);
BOTH(4) BOTH(8) BOTH(16) BOTH(32) BOTH(64)
void* the_walk() { return reinterpret_cast<void*>(&voltrix::random_walk_kernel); }
'''


def test_every_kernel_compiles_without_scratch_or_spills(tmp_path):
    # the report's remark lines are what profiles/subgraph/resource_usage.txt holds
    usage, _ = resource_usage(SOURCE, tmp_path, "subgraph", ("subgraph_kernel", "random_walk_kernel"))
    # count and fill in five widths, and the walk.  No LDS anywhere: the compaction goes through the ballot
    assert len(usage) == 11 and len([n for n in usage if "subgraph_kernel" in n]) == 10, sorted(usage)
    assert all(v == (0, 0, 0, 0) for v in usage.values()), usage
