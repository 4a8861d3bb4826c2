"""CPU: the weighted neighbour sampling rule and its plumbing.  The numpy restatement
(tests/weighted_sample_oracle.py) reproduces committed answers and hand-computed tables and draws with the probabilities of successive
sampling; a stand-alone host program runs the header's own ``weighted_sample_row`` -- the code the kernel runs -- on every row of the
GPU tests' graph and agrees with the oracle position by position; the C symbol is declared and bound, and its argument checks are a row of
tests/core_abi_cases.py; the Python layer raises before it looks at a tensor; both kernels compile for gfx950 without scratch and without
spilled registers.  No GPU compute is called here (tests/test_gpu_weighted_sample.py compares the kernels with the same oracle)."""
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO

import weighted_sample_oracle as oracle
from kernel_resources import resource_usage
from voltrix import capi

INCLUDE = os.path.join(REPO, "voltrix-spmm_amd", "voltrix", "include")
NAME = "voltrix_sample_neighbors_weighted"
ONE = 1 << 30

#        (r, q of the row, k, without replacement, with replacement) at seed 9, offset 0
KNOWN = ((5, [8, 4, 2, 1, 0, 7, 3], 3, [0, 1, 5], [1, 0, 3]),
         (77, list(range(1, 41)), 10, [7, 15, 25, 27, 30, 31, 34, 36, 37, 39], [36, 32, 39, 35, 27, 8, 29, 37, 34, 18]),
         (123456, [ONE] * 8 + [0, 5, 1], 4, [0, 1, 5, 7], [5, 7, 2, 0]),
         (2 ** 31 - 1, [1, ONE, 1, 1, 1, 1], 2, [1, 4], [1, 1]))


def test_known_answers():
    assert oracle.draws64([5], 2, 9, 0)[0] == [0x6CBED80DF8A08E97, 0x327713D4EECC5B6F]
    for r, q, k, want, want_replace in KNOWN:
        assert oracle.row_positions(q, r, k, 9, 0, False) == want, r
        assert oracle.row_positions(q, r, k, 9, 0, True) == want_replace, r
        assert oracle.row_positions(q, r, None, 9, 0, False) == [j for j, v in enumerate(q) if v > 0]
    # p <= k: every positive entry, no draw; T == 0: nothing, with and without replacement
    assert oracle.row_positions([0, 3, 0, 4, 0], 1, 2, 9, 0, False) == [1, 3] == oracle.row_positions([0, 3, 0, 4, 0], 1, 5, 9, 0, False)
    assert oracle.row_positions([0, 0], 1, 2, 9, 0, False) == [] == oracle.row_positions([0, 0], 1, 2, 9, 0, True)
    # the draws carry bits 31 and 29 in counter word 1: not the uniform rule's words for the same (seed, offset, row)
    import sample_oracle

    uniform = sample_oracle.draws([5, 77], 64, 9, 0).tolist()
    mine = [[half for x in row for half in (x >> 32, x & 0xFFFFFFFF)] for row in oracle.draws64([5, 77], 32, 9, 0)]
    assert not set(uniform[0]) & set(mine[0]) and not set(uniform[1]) & set(mine[1])


# ---- the table rule on a 12-row graph, q computed by hand
TABLE_ROWS = (([], []),                                                    # an empty row
              ([0, 0, 0], [0, 0, 0]),                                      # only zero weights
              ([0, 5.0, 0], [0, ONE, 0]),                                  # a single positive entry
              ([1, 1e-12], [ONE, 1]),                                      # floor(1e-12 2^30) = 0: the floor of 1 keeps it positive
              ([2, 1, 0.5, 0.25], [ONE, ONE >> 1, ONE >> 2, ONE >> 3]),
              ([3, 1], [ONE, 357913941]),                                  # floor(2^30 / 3)
              ([0.1, 0.2], [ONE >> 1, ONE]),                               # the same significand: exactly one half, in fp32 and in fp64
              ([7], [ONE]),
              ([1.5, 0, 3], [ONE >> 1, 0, ONE]),
              ([], []),
              ([1e30, 1e-30], [ONE, 1]),
              ([0.75, 1], [3 * (ONE >> 2), ONE]))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_table_rule_on_hand_computed_rows(dtype):
    assert len(TABLE_ROWS) == 12
    indptr = np.concatenate([[0], np.cumsum([len(w) for w, _ in TABLE_ROWS])])
    prob = np.array([v for w, _ in TABLE_ROWS for v in w], dtype=dtype)
    want = np.array([v for _, q in TABLE_ROWS for v in q], dtype=np.int64)
    q, cum, positive = oracle.weight_table(indptr, prob)
    assert q.dtype == np.int64 and np.array_equal(q, want)
    assert cum.dtype == np.int64 and np.array_equal(cum, np.cumsum(want)) and positive.dtype == np.int32
    assert positive.tolist() == [0, 0, 1, 2, 4, 2, 2, 1, 2, 0, 2, 2]
    assert q.min() == 0 and q.max() == ONE
    for bad in (-1.0, np.inf, np.nan):
        with pytest.raises(AssertionError):
            oracle.quantise([0, 2], np.array([1.0, bad]))


def test_successive_sampling_draws_every_subset_with_its_probability():
    """40,000 rows with q proportional to (8, 4, 2, 1).  Without replacement, k = 2: the subset {a, b} has probability
    pa pb / (1 - pa) + pa pb / (1 - pb) (a first or b first); every one of the six counts within 5 sigma (binomial) of it.  With
    replacement, k = 4: position counts within 5 sigma of n k q / T.  The multiply-high's bias, below 2^-63 per entry, is far below a
    sigma."""
    rows = np.arange(1000, 41000)
    n = rows.size
    q = [8 << 27, 4 << 27, 2 << 27, 1 << 27]
    p = np.array(q) / sum(q)
    counts = {pair: 0 for pair in itertools.combinations(range(4), 2)}
    for x in oracle.draws64(rows, 2, 20261020, 3):
        counts[tuple(oracle.successive_positions(q, x))] += 1
    assert sum(counts.values()) == n
    for (a, b), seen in counts.items():
        prob = p[a] * p[b] / (1 - p[a]) + p[a] * p[b] / (1 - p[b])
        deviation = abs(seen - n * prob) / (n * prob * (1 - prob)) ** 0.5
        print(f"subset {a, b}: {seen} of {n}, expected {n * prob:.1f}, {deviation:.2f} sigma")
        assert deviation <= 5, (a, b, seen, deviation)
    k = 4
    positions = np.array([oracle.replace_positions(q, x) for x in oracle.draws64(rows, k, 20261020, 3)])
    seen = np.bincount(positions.ravel(), minlength=4)
    deviation = np.abs(seen - n * k * p) / (n * k * p * (1 - p)) ** 0.5
    print(f"with replacement: counts {seen.tolist()}, deviations {np.round(deviation, 2).tolist()} sigma")
    assert seen.sum() == n * k and (deviation <= 5).all(), (seen, deviation)


# ---- the header's own row function in a host program, on every row of the GPU tests' graph
PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <vector>

#include "voltrix/weighted_sample_kernels.hpp"

struct ArraySlots {
  std::vector<int> v;
  int get(int j) const { return v.at(j); }
  void set(int j, int x) { v.at(j) = x; }
};

template <bool REPLACE>
static int run(char tag, const std::vector<long long>& cum, int begin, int d, unsigned long long r, int k, int room,
               unsigned long long seed, unsigned long long offset) {
  std::printf("%c", tag);
  if (d > 0 && room > 0) {
    // the row in buffers of its own, so that the host's sanitizer sees a read outside the row, of cum[-1] for a row that begins at
    // entry 0 included, a write past the row's segment and a slot past k
    const int first = begin > 0 ? 1 : 0;
    std::vector<long long> mass(cum.begin() + (begin - first), cum.begin() + (begin + d));
    std::vector<int> cols(first + d), out_col(room, -1), out_entry(room, -1);
    for (int j = 0; j < first + d; ++j) cols[j] = 1000 + j;
    ArraySlots slot{std::vector<int>(k == INT_MAX ? 0 : k, -1)};
    voltrix::weighted_sample_row<REPLACE>(cols.data(), mass.data(), (uint32_t)r, first, d, k, room, (uint32_t)seed,
                                          (uint32_t)(seed >> 32), (uint32_t)offset, (uint32_t)(offset >> 32), slot, out_col.data(),
                                          out_entry.data());
    for (int j = 0; j < room; ++j) {
      if (out_col[j] != 1000 + out_entry[j]) return 6;
      std::printf(" %d", out_entry[j] - first);
    }
  }
  std::printf("\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  long long num_rows = 0, nnz = 0, num_cases = 0;
  in >> num_rows >> nnz;
  std::vector<int> indptr(num_rows + 1);
  std::vector<long long> cum(nnz);
  for (auto& v : indptr) in >> v;
  for (auto& v : cum) in >> v;
  in >> num_cases;
  std::printf("lds %zu %zu %zu %zu %zu\n", voltrix::weighted_sample_lds_bytes(1, 0), voltrix::weighted_sample_lds_bytes(64, 0),
              voltrix::weighted_sample_lds_bytes(10, 1), voltrix::weighted_sample_lds_bytes(voltrix::kSampleAll, 0),
              voltrix::weighted_sample_lds_bytes(voltrix::kSampleAll, 1));
  for (long long n = 0; n < num_cases; ++n) {
    unsigned long long r = 0, seed = 0, offset = 0;
    int k = 0, room = 0, room_replace = 0;
    in >> r >> k >> room >> room_replace >> seed >> offset;
    if (!in) return 3;
    const int begin = indptr[r], d = indptr[r + 1] - begin, fanout = k < 0 ? INT_MAX : k;
    if (int rc = run<false>('f', cum, begin, d, r, fanout, room, seed, offset)) return rc;
    if (int rc = run<true>('r', cum, begin, d, r, fanout, room_replace, seed, offset)) return rc;
  }
  return 0;
}
"""

STREAMS = ((20261020, 2 ** 32 + 7), (2 ** 64 - 1, 2 ** 64 - 1))


def test_host_and_device_run_the_same_row_function(tmp_path):
    indptr, _, prob, _ = oracle.build_graph()
    q, cum, positive = oracle.weight_table(indptr, prob)
    cases = [(r, k, seed, offset) for (seed, offset), k in itertools.product(STREAMS, oracle.FANOUTS) for r in range(oracle.NUM_ROWS)]
    lines = [f"{oracle.NUM_ROWS} {cum.size}", " ".join(map(str, indptr.tolist())), " ".join(map(str, cum.tolist())), str(len(cases))]
    for r, k, seed, offset in cases:
        p = int(positive[r])
        room, room_replace = (p, p) if k is None else (min(p, k), k if p else 0)
        lines.append(f"{r} {-1 if k is None else k} {room} {room_replace} {seed} {offset}")
    table, src, exe = tmp_path / "table.txt", tmp_path / "main.hip", tmp_path / "main"
    table.write_text("\n".join(lines) + "\n")
    src.write_text(PROGRAM)
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    # the header as HIP (its kernels are compiled for gfx950 and not launched: the program makes no HIP runtime call); the sanitizers
    # are the host's and check the stand-alone program
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", "-Wall", "-Werror", "-Xarch_host", "-fsanitize=address",
                           "-Xarch_host", "-fsanitize=undefined", "-fno-sanitize-recover=all", f"-I{INCLUDE}", str(src), "-o", str(exe)])
    out = subprocess.run([str(exe), str(table)], check=True, capture_output=True, text=True).stdout.splitlines()
    # the launch's dynamic LDS: 256 k 4 bytes without replacement, none with it or for "all"
    assert out[0] == f"lds {256 * 4} {256 * 64 * 4} 0 0 0"
    assert len(cases) == 3000 and len(out) == 1 + 2 * len(cases)
    for n, (r, k, seed, offset) in enumerate(cases):
        row = q[indptr[r]:indptr[r + 1]]
        for line, tag, replace in ((out[1 + 2 * n], "f", False), (out[2 + 2 * n], "r", True)):
            assert line[0] == tag and [int(v) for v in line.split()[1:]] == oracle.row_positions(row, r, k, seed, offset, replace), \
                (r, k, seed, offset, replace)


# ---- plumbing
def test_header_declares_and_binding_lists_the_symbol():
    import voltrix

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "voltrix_capi.h")).read(), flags=re.S)
    assert re.search(rf"\b{NAME}\s*\(", text)
    assert NAME in capi.SYMBOLS and NAME in capi.SIGNATURES and hasattr(capi.lib(), NAME)
    assert not NAME.startswith("voltrix_launch_")            # in the launchers' contract table by its signature, not by its name
    assert capi.lib().voltrix_abi_version() == 2
    assert callable(voltrix.sampling_weights) and voltrix.SamplingWeights is voltrix.sampling.SamplingWeights
    assert not hasattr(capi.sample_neighbors_weighted, "timer_label")


def test_python_layer_rejects_prob_misuse_before_any_tensor_is_looked_at():
    import torch

    import voltrix

    weights = voltrix.SamplingWeights(None, None, 0, 0)
    plain = torch.ones(4)
    with pytest.raises(ValueError, match="sampling_weights"):                # the weights themselves, not their table
        voltrix.sample_neighbors(None, None, None, 10, 1, prob=plain)
    with pytest.raises(ValueError, match="sampling_weights"):
        voltrix.sample_blocks(None, None, None, (10, 5), 1, prob=plain)
    with pytest.raises(ValueError, match="exclude"):
        voltrix.sample_neighbors(None, None, None, 10, 1, exclude=plain, prob=weights)
    with pytest.raises(ValueError, match="exclude"):
        voltrix.sample_blocks(None, None, None, (10, 5), 1, exclude=plain, prob=weights)
    with pytest.raises(ValueError):                                          # tensors are looked at next: a host tensor is no device CSR
        voltrix.sampling_weights(torch.zeros(3, dtype=torch.int32), plain)


SOURCE = r'''
#include "voltrix/weighted_sample_kernels.hpp"
template __global__ void voltrix::sample_neighbors_weighted_kernel<false>(const voltrix::WeightedSampleArgs);
template __global__ void voltrix::sample_neighbors_weighted_kernel<true>(const voltrix::WeightedSampleArgs);
'''


def test_both_kernels_compile_without_scratch_or_spills(tmp_path):
    usage, _ = resource_usage(SOURCE, tmp_path, "weighted", ("sample_neighbors_weighted_kernel",))
    # with and without replacement.  The static LDS is 0 (a promoted per-lane array would show here); the dynamic LDS is the launch's,
    # 256 k 4 bytes without replacement only (weighted_sample_lds_bytes, printed by the host program above)
    assert len(usage) == 2, sorted(usage)
    assert all(v == (0, 0, 0, 0) for v in usage.values()), usage
