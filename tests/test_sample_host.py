"""CPU: the neighbour sampling rule and its plumbing.  The numpy restatement (tests/sample_oracle.py) reproduces the
known answers and draws uniformly; a stand-alone host program runs the header's own ``sample_row`` -- the code the kernel runs, here
the instantiation of a launch without an exclusion list (tests/test_exclude_host.py runs the other, with and without a list) -- and
agrees with it line by line; the four entry points are declared, bound and exported; their argument checks are rows of
tests/core_abi_cases.py; the Python layer raises before it looks at a tensor; every kernel compiles for gfx950 without scratch and
without spilled registers.  No GPU compute is called here (tests/test_gpu_sample.py compares the kernels with the same oracle)."""
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO

import sample_oracle as oracle
from kernel_resources import resource_usage
from voltrix import capi

HEADER = os.path.join(REPO, "include", "voltrix_capi.h")
INCLUDE = os.path.join(REPO, "voltrix-spmm_amd", "voltrix", "include")
NAMES = ("voltrix_launch_sample_neighbors", "voltrix_launch_block_mark", "voltrix_launch_block_mark_seeds",
         "voltrix_launch_block_relabel")

KNOWN = ((5, 40, [11, 19, 20, 25, 27, 28, 29, 33, 34, 38]),
         (77, 50, [3, 4, 7, 13, 18, 19, 20, 37, 42, 43]),
         (123456, 60, [0, 14, 17, 19, 23, 26, 44, 45, 46, 54]))


def test_known_answers():
    for row, degree, want in KNOWN:
        assert oracle.floyd_positions([row], [degree], 10, 9, 0)[0].tolist() == want, row
    rows, degrees = [k[0] for k in KNOWN], [k[1] for k in KNOWN]                         # vectorised = row by row
    assert oracle.floyd_positions(rows, degrees, 10, 9, 0).tolist() == [k[2] for k in KNOWN]
    # the draws carry bit 31 in counter word 1: not the dropout mask's words for the same (seed, offset, first counter word)
    from test_attn_dropout_host import philox4x32_10

    mask_words = np.stack(philox4x32_10(np.array(rows), 0, 0, 0, 9, 0), -1)
    assert not (oracle.draws(rows, 4, 9, 0) == mask_words).any()


@pytest.mark.parametrize("degree,k", [(11, 10), (37, 10), (64, 25), (5, 1), (300, 32)])
def test_the_rule_draws_every_subset_position_equally(degree, k):
    """Inclusion counts of every position within 5 sigma of n k / d (binomial sigma), and the joint inclusion of positions 0 and d - 1
    within 5 sigma of k (k - 1) / (d (d - 1)): the margin of test_kept_fraction_is_one_minus_p.  The multiply-shift's bias, at most
    d / 2^32 < 1e-7 relative, is four orders of magnitude below one sigma at n = 40,000."""
    rows = np.arange(1000, 41000)
    n = rows.size
    positions = oracle.floyd_positions(rows, degree, k, 20261019, 3)
    assert (np.diff(positions, axis=1) > 0).all() and positions.min() >= 0 and positions.max() < degree     # k distinct, ascending
    p = k / degree
    counts = np.bincount(positions.ravel(), minlength=degree)
    worst = np.abs(counts - n * p).max() / (n * p * (1 - p)) ** 0.5
    print(f"d={degree} k={k}: worst inclusion deviation {worst:.2f} sigma")
    assert worst <= 5, (degree, k, worst)
    if k >= 2:
        q = k * (k - 1) / (degree * (degree - 1))
        both = int(((positions[:, 0] == 0) & (positions[:, -1] == degree - 1)).sum())
        joint = abs(both - n * q) / (n * q * (1 - q)) ** 0.5
        print(f"d={degree} k={k}: joint inclusion of 0 and d-1 deviates {joint:.2f} sigma")
        assert joint <= 5, (degree, k, joint)


def test_oracle_sample_neighbors_and_blocks_on_a_small_graph():
    rng = np.random.default_rng(0)
    degrees = np.array([0, 1, 2, 3, 4, 7, 30, 5, 0, 9, 3, 3])
    indptr = np.concatenate([[0], np.cumsum(degrees)])
    indices = rng.integers(0, 12, indptr[-1])
    seeds = np.array([6, 0, 3, 9, 1])
    ip, cols, entries = oracle.sample_neighbors(indptr, indices, seeds, 3, 7, 2)
    assert np.diff(ip).tolist() == [3, 0, 3, 3, 1] and np.array_equal(cols, indices[entries])
    for i, r in enumerate(seeds):
        mine = entries[ip[i]:ip[i + 1]]
        assert (np.diff(mine) > 0).all() and (mine >= indptr[r]).all() and (mine < indptr[r + 1]).all()
    assert np.array_equal(entries[ip[2]:ip[3]], np.arange(indptr[3], indptr[4]))         # d == k: the row as it is
    one = oracle.sample_neighbors(indptr, indices, [6], 3, 7, 2)                         # a row's sample does not depend on its batch
    assert np.array_equal(one[2], entries[:3])
    ip_r, cols_r, entries_r = oracle.sample_neighbors(indptr, indices, seeds, 3, 7, 2, replace=True)
    assert np.diff(ip_r).tolist() == [3, 0, 3, 3, 3] and (entries_r[-3:] == indptr[1]).all()      # degree 1: the one entry, k times
    ip_a, _, entries_a = oracle.sample_neighbors(indptr, indices, seeds, None, 7, 2)
    assert np.diff(ip_a).tolist() == degrees[seeds].tolist()
    assert np.array_equal(entries_a, np.concatenate([np.arange(indptr[r], indptr[r + 1]) for r in seeds]))
    src, local = oracle.compact_block(seeds, cols)
    assert np.array_equal(src[:5], seeds) and (np.diff(src[5:]) > 0).all() and not set(src[5:]) & set(seeds)
    assert np.array_equal(src[local], cols)
    blocks = oracle.sample_blocks(indptr, indices, seeds, (3, 2), 7, 10)
    assert len(blocks) == 2 and np.array_equal(blocks[1]["dst_ids"], seeds) and np.array_equal(blocks[0]["dst_ids"], blocks[1]["src_ids"])
    assert np.array_equal(blocks[1]["entries"], oracle.sample_neighbors(indptr, indices, seeds, 2, 7, 10)[2])          # l = 0
    assert np.array_equal(blocks[0]["entries"], oracle.sample_neighbors(indptr, indices, blocks[1]["src_ids"], 3, 7, 11)[2])


# ---- the header's own selection code in a host program
PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "voltrix/neighbor_sample_kernels.hpp"

struct ArraySlots {
  std::vector<int> v;
  int get(int j) const { return v.at(j); }
  void set(int j, int x) { v.at(j) = x; }
};

int main(int argc, char** argv) {
  for (int i = 1; i + 4 < argc; i += 5) {
    const unsigned long long r = std::strtoull(argv[i], nullptr, 10), seed = std::strtoull(argv[i + 3], nullptr, 10),
                             offset = std::strtoull(argv[i + 4], nullptr, 10);
    const int d = std::atoi(argv[i + 1]), k = std::atoi(argv[i + 2]);
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32), off0 = (uint32_t)offset, off1 = (uint32_t)(offset >> 32);
    // the row function without a list, on a row that begins at entry 0 and whose columns are its positions: entry ids = positions
    std::vector<int> row(d), cols(k), entries(k);
    for (int j = 0; j < d; ++j) row[j] = j;
    ArraySlots slot{std::vector<int>(k, -1)};
    voltrix::sample_row<false, false>(row.data(), nullptr, 0, (uint32_t)r, 0, d, k, k, k0, k1, off0, off1, slot, cols.data(),
                                      entries.data());
    if (cols != entries) return 6;
    std::printf("f");
    for (int j = 0; j < k; ++j) std::printf(" %d", entries[j]);
    voltrix::sample_row<true, false>(row.data(), nullptr, 0, (uint32_t)r, 0, d, k, k, k0, k1, off0, off1, slot, cols.data(),
                                     entries.data());
    if (cols != entries) return 6;
    std::printf("\nr");
    for (int j = 0; j < k; ++j) std::printf(" %d", entries[j]);
    std::printf("\n");
  }
  return 0;
}
"""

FANOUTS = (1, 2, 10, 25, 63, 64)
ROWS = (0, 5, 123456, 2 ** 31 - 2, 2 ** 31 - 1)
STREAMS = ((9, 0), (20261019, 3), (2 ** 63 + 1, 2 ** 32 + 5), (2 ** 64 - 1, 2 ** 64 - 1))
#         (r, d, k, seed, offset): d = k + 1, d a little above, d = 67,000, for every fan-out, row and stream
CASES = [(r, d, k, seed, offset) for k, r, (seed, offset) in itertools.product(FANOUTS, ROWS, STREAMS) for d in (k + 1, 2 * k + 3, 67000)]


def test_host_and_device_run_the_same_selection_code(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src, exe = tmp_path / "main.hip", tmp_path / "main"
    src.write_text(PROGRAM)
    # the header as HIP (its kernels are compiled for gfx950 and not launched: the program makes no HIP runtime call); the sanitizers
    # are the host's and check the stand-alone program
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", "-Wall", "-Werror", "-Xarch_host", "-fsanitize=address",
                           "-Xarch_host", "-fsanitize=undefined", "-fno-sanitize-recover=all", f"-I{INCLUDE}", str(src), "-o", str(exe)])
    assert len(CASES) == 360
    args = [str(v) for case in CASES for v in case]
    lines = subprocess.run([str(exe)] + args, check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(lines) == 2 * len(CASES)
    for n, (r, d, k, seed, offset) in enumerate(CASES):
        floyd = [int(v) for v in lines[2 * n].split()[1:]]
        assert lines[2 * n][0] == "f" and floyd == oracle.floyd_positions([r], [d], k, seed, offset)[0].tolist(), (r, d, k, seed, offset)
        replace = [int(v) for v in lines[2 * n + 1].split()[1:]]
        assert replace == oracle.replace_positions([r], [d], k, seed, offset)[0].tolist(), (r, d, k, seed, offset)


# ---- plumbing
def test_header_declares_and_binding_lists_the_entry_points():
    import voltrix

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in capi.SYMBOLS and name in capi.SIGNATURES, name
        assert hasattr(capi.lib(), name)
    assert capi.lib().voltrix_abi_version() == 2
    for fn in (voltrix.sample_neighbors, voltrix.compact_block, voltrix.sample_blocks):
        assert callable(fn)
    assert voltrix.Block is voltrix.sampling.Block and (capi.SAMPLE_ALL, capi.SAMPLE_MAX_FANOUT) == (-1, 64)
    for wrapper in ("launch_sample_neighbors", "launch_block_mark", "launch_block_mark_seeds", "launch_block_relabel"):
        assert not hasattr(getattr(capi, wrapper), "timer_label"), wrapper


def test_python_layer_rejects_bad_arguments_before_any_tensor_is_looked_at():
    import voltrix

    for fanout in (0, 65, -1, 2.0, "10", True):
        with pytest.raises(ValueError):
            voltrix.sample_neighbors(None, None, None, fanout, 1)
        with pytest.raises(ValueError):
            voltrix.sample_blocks(None, None, None, (10, fanout), 1)
    for seed, offset in ((-1, 0), (2 ** 64, 0), (0, -1), (0, 2 ** 64), (1.5, 0), (0, None)):
        with pytest.raises(ValueError):
            voltrix.sample_neighbors(None, None, None, 10, seed, offset)
        with pytest.raises(ValueError):
            voltrix.sample_blocks(None, None, None, (10, None), seed, offset)
    import torch

    host = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError):                          # tensors are looked at next: a host tensor is not a device CSR
        voltrix.sample_neighbors(host, host, host, 10, 1)
    with pytest.raises(ValueError):
        voltrix.compact_block(host, host, 4)


SOURCE = r'''
#include "voltrix/neighbor_sample_kernels.hpp"
template __global__ void voltrix::sample_neighbors_kernel<false, false>(const voltrix::SampleNeighborsArgs);
template __global__ void voltrix::sample_neighbors_kernel<true, false>(const voltrix::SampleNeighborsArgs);
template __global__ void voltrix::sample_neighbors_kernel<false, true>(const voltrix::SampleNeighborsArgs);
template __global__ void voltrix::sample_neighbors_kernel<true, true>(const voltrix::SampleNeighborsArgs);
void* the_mark() { return reinterpret_cast<void*>(&voltrix::block_mark_kernel); }
void* the_mark_seeds() { return reinterpret_cast<void*>(&voltrix::block_mark_seeds_kernel); }
void* the_relabel() { return reinterpret_cast<void*>(&voltrix::block_relabel_kernel); }
'''


def test_every_kernel_compiles_without_scratch_or_spills(tmp_path):
    keys = ("sample_neighbors_kernel", "block_mark_kernel", "block_mark_seeds_kernel", "block_relabel_kernel")
    usage, _ = resource_usage(SOURCE, tmp_path, "sample", keys)
    # with and without replacement, each without and with an exclusion list, and the three relabelling kernels.  The static LDS is 0
    # everywhere (a promoted per-lane array would show here); the dynamic LDS of the kernels without replacement is the launch's,
    # 256 k 4 bytes
    assert len(usage) == 7 and len([n for n in usage if "sample_neighbors_kernel" in n]) == 4, sorted(usage)
    assert all(v == (0, 0, 0, 0) for v in usage.values()), usage
