"""CPU: the negative-sampling rule, the entry -> endpoints search and their plumbing.  The numpy restatement
(tests/negative_oracle.py) reproduces the known answers written out here, in the kernel header and in DESIGN.md, draws from a counter
domain of its own, samples the non-neighbours uniformly and never a neighbour; a stand-alone host program runs the header's own
``negative_pick`` / ``entry_row`` -- the code the kernels run -- and agrees with it, sorted and unsorted; the two entry points are
declared, bound and exported; their argument checks are rows of tests/core_abi_cases.py; the Python layer raises before it looks at
a tensor; both kernels, in both ``SORTED`` instantiations, compile for gfx950 without scratch, spilled registers or LDS.  No GPU
compute is called here (tests/test_gpu_negative.py compares the kernels with the same oracle)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO

import negative_oracle as oracle
from kernel_resources import resource_usage
from voltrix import capi

HEADER = os.path.join(REPO, "include", "voltrix_capi.h")
INCLUDE = os.path.join(REPO, "voltrix-spmm_amd", "voltrix", "include")
NAMES = ("voltrix_launch_negative_sample", "voltrix_launch_edge_endpoints")
SRC = [0, 0, 5, 99]


def _ring():
    """100 nodes, row v = [(v + 1) % 100, (v + 7) % 100, (v + 31) % 100] (tests/test_subgraph_host.py): not every row ascends."""
    n = 100
    return np.arange(0, 3 * n + 1, 3), np.array([[(v + 1) % n, (v + 7) % n, (v + 31) % n] for v in range(n)]).ravel()


def _band():
    """100 nodes, row v = {v + 1 .. v + 60} mod 100, ascending: 40 non-neighbours, so most tries are rejected."""
    n = 100
    return np.arange(0, 60 * n + 1, 60), np.array([np.sort((v + 1 + np.arange(60)) % n) for v in range(n)]).ravel()


def _sorted_rows(indptr, indices):
    return indptr, np.concatenate([np.sort(indices[a:b]) for a, b in zip(indptr[:-1], indptr[1:])] + [np.zeros(0, indices.dtype)])


def _gaps():
    """12 rows with runs of empty rows in front, inside and at the end; one column outside [0, 12)."""
    degrees = np.array([0, 0, 3, 0, 0, 0, 2, 1, 0, 4, 0, 0])
    indptr = np.concatenate([[0], np.cumsum(degrees)])
    return indptr, np.array([1, 4, 9, 0, 11, 5, 2, 3, 7, 40])


# ---- the rule
def test_known_answers_of_the_negative_rule():
    ring, band = _ring(), _band()
    neg, exhausted = oracle.negative_sample(*ring, SRC, 4, 9, 0)
    assert neg.tolist() == [[38, 49, 82, 73], [29, 70, 90, 20], [99, 4, 63, 22], [21, 68, 11, 37]] and exhausted == 0
    assert neg.dtype == np.int32 and neg[0].tolist() != neg[1].tolist()                 # the same source, another position
    high, _ = oracle.negative_sample(*ring, SRC, 4, 2 ** 40 + 9, 2 ** 32 + 7)           # the high words of seed and offset
    assert high.tolist() == [[24, 42, 80, 16], [72, 50, 67, 9], [40, 60, 94, 56], [66, 95, 96, 73]]
    # T = 5, k = 3: the slots start at q = 0, 5 and 10 -- q & 3 = 0, 1, 2 -- and each crosses a Philox block boundary
    proposals = ((oracle.draws([0], 0, 15, 9, 0) * np.uint64(100)) >> np.uint64(32))[0].tolist()
    assert proposals == [38, 36, 7, 67, 86, 2, 77, 74, 86, 4, 16, 32, 5, 47, 37]         # row 0 holds 1 .. 60
    neg, exhausted = oracle.negative_sample(*band, SRC, 3, 9, 0, None, 5)
    assert neg.tolist() == [[67, 77, -1], [62, 74, 66], [99, 67, 83], [66, 71, 63]] and exhausted == 1
    high, exhausted = oracle.negative_sample(*band, SRC, 3, 2 ** 40 + 9, 2 ** 32 + 7, None, 5)
    assert high.tolist() == [[96, 91, 79], [72, 71, 85], [66, 1, 85], [66, 71, 77]] and exhausted == 0


def test_a_slot_does_not_depend_on_k_or_on_the_other_sources():
    band = _band()
    wide, _ = oracle.negative_sample(*band, SRC, 7, 9, 3, None, 5)
    narrow, _ = oracle.negative_sample(*band, SRC, 3, 9, 3, None, 5)
    assert np.array_equal(wide[:, :3], narrow)
    other, _ = oracle.negative_sample(*band, [42, 0, 17, 99], 3, 9, 3, None, 5)         # positions 1 and 3 keep their sources
    assert np.array_equal(other[[1, 3]], narrow[[1, 3]]) and not np.array_equal(other[[0, 2]], narrow[[0, 2]])
    fewer, _ = oracle.negative_sample(*band, SRC, 3, 9, 3, None, 4)                     # another T: other draws from slot 1 on
    assert np.array_equal(fewer[:, 0] >= 0, fewer[:, 0] == narrow[:, 0]) and not np.array_equal(fewer, narrow)


def test_the_draws_have_a_counter_domain_of_their_own():
    """Bit 30 set, bit 31 clear: not the dropout mask's words (00), not the neighbour sampler's (10), not the walk's (11), for the same
    (seed, offset, index)."""
    import sample_oracle
    import subgraph_oracle
    from test_attn_dropout_host import philox4x32_10

    index = np.arange(4)
    mine = oracle.draws(index, 0, 4, 9, 0)
    assert oracle.COUNTER_BITS == 0x40000000 and sample_oracle.COUNTER_BIT == 0x80000000 and subgraph_oracle.COUNTER_BITS == 0xC0000000
    assert not (mine == np.stack(philox4x32_10(index, 0, 0, 0, 9, 0), -1)).any()
    assert not (mine == sample_oracle.draws(index, 4, 9, 0)).any()
    assert not (mine == subgraph_oracle.walk_draws(index, 4, 9, 0)).any()
    # and the domain is what separates them: the same block without the bits is the mask's
    assert np.array_equal(np.stack(philox4x32_10(index, 0x40000000, 0, 0, 9, 0), -1).astype(np.uint64), mine)
    # a slot that starts mid-block reads the block's later words: draws 5 .. 9 are words 1, 2, 3 of block 1 and 0, 1 of block 2
    assert np.array_equal(oracle.draws(index, 5, 5, 9, 0), oracle.draws(index, 0, 12, 9, 0)[:, 5:10])


def test_every_non_neighbour_is_drawn_equally_and_no_neighbour_ever():
    """40,000 positions on one row of degree 16 in a 64-column graph, k = 1: every non-neighbour's count within 5 sigma of n / 48
    (binomial sigma).  The multiply-shift's bias, at most 64 / 2^32 relative, is orders of magnitude below one sigma."""
    n, cols = 40000, 64
    neighbours = np.sort(np.random.default_rng(7).choice(cols, 16, replace=False))
    indptr, indices = np.array([0, 16]), neighbours
    neg, exhausted = oracle.negative_sample(indptr, indices, np.zeros(n, np.int64), 1, 20261019, 3, cols)
    assert exhausted == 0 and neg.shape == (n, 1)                                        # 0.25^16 per slot
    counts = np.bincount(neg[:, 0], minlength=cols)
    assert (counts[neighbours] == 0).all()
    others = np.setdiff1d(np.arange(cols), neighbours)
    p = 1 / 48
    worst = np.abs(counts[others] - n * p).max() / (n * p * (1 - p)) ** 0.5
    print(f"worst deviation {worst:.2f} sigma")
    assert others.size == 48 and counts[others].sum() == n and worst <= 5, worst


def test_exclude_self():
    """A square graph without entries and four columns: a quarter of the first proposals is the source itself."""
    indptr, indices, src = np.zeros(5, np.int64), np.zeros(0, np.int64), np.arange(400) % 4
    plain, _ = oracle.negative_sample(indptr, indices, src, 2, 9, 1)
    strict, exhausted = oracle.negative_sample(indptr, indices, src, 2, 9, 1, None, 16, True)
    own = plain == src[:, None]
    assert 120 < own.sum() < 280 and not (strict == src[:, None]).any() and exhausted == 0
    assert np.array_equal(plain[~own], strict[~own])                                    # the first try was accepted in both
    # one column: the source is the only proposal there is
    only, exhausted = oracle.negative_sample(np.zeros(2, np.int64), indices, [0, 0, 0], 2, 9, 1, None, 3, True)
    assert (only == -1).all() and exhausted == 6
    # a full row is exhausted with or without; the empty row next to it accepts its first proposals
    for flag in (False, True):
        full, exhausted = oracle.negative_sample(np.array([0, 4, 4, 4, 4]), np.arange(4), [0, 1], 3, 9, 1, None, 16, flag)
        assert full[0].tolist() == [-1, -1, -1] and (full[1] >= 0).all() and exhausted == 3


def test_entries_outside_the_columns_never_match_and_endpoints_skip_empty_rows():
    indptr, indices = _gaps()
    rows, cols = oracle.edge_endpoints(indptr, indices, [0, 2, 3, 4, 5, 6, 9, -1, 10, 2 ** 31 - 1])
    assert rows.tolist() == [2, 2, 6, 6, 7, 9, 9, -1, -1, -1] and cols.tolist() == [1, 9, 0, 11, 5, 2, 40, -1, -1, -1]
    # row 9 holds 2, 3, 7 and a 40: with 12 columns the 40 is nobody's column, with 64 it is row 9's
    narrow, _ = oracle.negative_sample(indptr, indices, np.full(3000, 9), 1, 5, 0, 12)
    wide, _ = oracle.negative_sample(indptr, indices, np.full(3000, 9), 1, 5, 0, 64)
    assert set(narrow.ravel().tolist()) == set(range(12)) - {2, 3, 7} and set(wide.ravel().tolist()) == set(range(64)) - {2, 3, 7, 40}
    none, exhausted = oracle.negative_sample(indptr, indices, [9, 2], 4, 5, 0, 0)        # no columns: nothing to propose
    assert (none == -1).all() and exhausted == 8


# ---- the header's own code in a host program
PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "voltrix/negative_sample_kernels.hpp"

// argv: graph file (num_rows, indptr, the number of entries, indices), then
//   "pick" num_cols k tries exclude_self sorted seed offset src ...    -> one line of k columns per position
//   "rows" entries ...                                                 -> one row id per entry
int main(int argc, char** argv) {
  if (argc < 3) return 2;
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 3;
  int num_rows = 0, count = 0;
  if (std::fscanf(f, "%d", &num_rows) != 1) return 4;
  std::vector<int> indptr(num_rows + 1);
  for (int& v : indptr) if (std::fscanf(f, "%d", &v) != 1) return 4;
  if (std::fscanf(f, "%d", &count) != 1) return 4;
  std::vector<int> indices(count);            // exactly as large as the CSR: the host's sanitizer sees a read outside a row
  for (int& v : indices) if (std::fscanf(f, "%d", &v) != 1) return 4;
  std::fclose(f);
  if (!std::strcmp(argv[2], "rows")) {
    for (int i = 3; i < argc; ++i) std::printf("%d\n", voltrix::entry_row(indptr.data(), num_rows, count, std::atoi(argv[i])));
    return 0;
  }
  if (argc < 10) return 2;
  const int num_cols = std::atoi(argv[3]), k = std::atoi(argv[4]), tries = std::atoi(argv[5]);
  const bool exclude_self = std::atoi(argv[6]) != 0, sorted = std::atoi(argv[7]) != 0;
  const unsigned long long seed = std::strtoull(argv[8], nullptr, 10), offset = std::strtoull(argv[9], nullptr, 10);
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32), o0 = (uint32_t)offset, o1 = (uint32_t)(offset >> 32);
  for (int p = 0; p + 10 < argc; ++p) {
    const int r = std::atoi(argv[10 + p]);
    for (int j = 0; j < k; ++j) {
      const int c = sorted ? voltrix::negative_pick<true>(indptr.data(), indices.data(), num_rows, num_cols, (uint32_t)p, j, r, tries,
                                                          exclude_self, k0, k1, o0, o1)
                           : voltrix::negative_pick<false>(indptr.data(), indices.data(), num_rows, num_cols, (uint32_t)p, j, r, tries,
                                                           exclude_self, k0, k1, o0, o1);
      std::printf(j ? " %d" : "%d", c);
    }
    std::printf("\n");
  }
  return 0;
}
"""

#       (graph, num_cols, k, tries, exclude_self, seed, offset, src)
PICKS = [("ring", 100, 4, 16, 0, 9, 0, SRC), ("ring", 100, 4, 16, 0, 2 ** 40 + 9, 2 ** 32 + 7, SRC),
         ("band", 100, 3, 5, 0, 9, 0, SRC), ("band", 100, 3, 5, 1, 2 ** 40 + 9, 2 ** 32 + 7, SRC),
         ("band", 100, 5, 3, 1, 20261019, 3, list(range(100))), ("band", 100, 1, 17, 0, 2 ** 64 - 1, 2 ** 64 - 1, list(range(0, 100, 3))),
         ("ring", 100, 2, 1, 1, 5, 1, list(range(100))), ("gaps", 12, 6, 7, 0, 5, 0, list(range(12)) + [9, 9, -1, 12]),
         ("gaps", 64, 6, 2, 1, 5, 2 ** 32 + 5, list(range(12))), ("gaps", 1, 3, 4, 0, 5, 0, [0, 2, 9]), ("gaps", 0, 2, 4, 0, 5, 0, [2, 9])]


def test_host_and_device_run_the_same_selection_code(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src, exe = tmp_path / "main.hip", tmp_path / "main"
    src.write_text(PROGRAM)
    # the header as HIP (its kernels are compiled for gfx950 and not launched: the program makes no HIP runtime call); the sanitizers
    # are the host's and check the stand-alone program
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", "-Wall", "-Werror", "-Xarch_host", "-fsanitize=address",
                           "-Xarch_host", "-fsanitize=undefined", "-fno-sanitize-recover=all", f"-I{INCLUDE}", str(src), "-o", str(exe)])
    rng = np.random.default_rng(3)
    graphs = {"ring": _sorted_rows(*_ring()), "band": _band(), "gaps": _sorted_rows(*_gaps())}
    shuffled = {name: (ip, np.concatenate([rng.permutation(ix[a:b]) for a, b in zip(ip[:-1], ip[1:])] + [ix[:0]]))
                for name, (ip, ix) in graphs.items()}
    assert any((np.diff(shuffled["band"][1][:60]) < 0).tolist())
    for kind, table in (("sorted", graphs), ("shuffled", shuffled)):
        for name, (indptr, indices) in table.items():
            (tmp_path / f"{kind}_{name}").write_text(" ".join(str(int(v)) for v in [indptr.size - 1, *indptr, indices.size, *indices]))
    slots = 0
    for name, num_cols, k, tries, exclude_self, seed, offset, positions in PICKS:
        want, _ = oracle.negative_sample(*graphs[name], positions, k, seed, offset, num_cols, tries, bool(exclude_self))
        slots += want.size
        # the binary search on ascending rows, the scan on the same rows and the scan on shuffled rows: the same bits
        for kind, is_sorted in (("sorted", 1), ("sorted", 0), ("shuffled", 0)):
            run = subprocess.run([str(exe), str(tmp_path / f"{kind}_{name}"), "pick", str(num_cols), str(k), str(tries), str(exclude_self),
                                  str(is_sorted), str(seed), str(offset)] + [str(s) for s in positions],
                                 check=True, capture_output=True, text=True)
            got = [[int(v) for v in line.split()] for line in run.stdout.splitlines()]
            assert got == want.tolist(), (name, kind, is_sorted, seed)
    assert slots > 500
    for name, (indptr, indices) in graphs.items():
        entries = list(range(-2, indices.size + 2)) + [2 ** 31 - 1, -2 ** 31]
        run = subprocess.run([str(exe), str(tmp_path / f"sorted_{name}"), "rows"] + [str(e) for e in entries], check=True,
                             capture_output=True, text=True)
        assert [int(v) for v in run.stdout.split()] == oracle.edge_endpoints(indptr, indices, entries)[0].tolist(), name


# ---- plumbing
def test_header_declares_and_binding_lists_the_entry_points():
    import voltrix

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in capi.SYMBOLS and name in capi.SIGNATURES, name
        assert hasattr(capi.lib(), name)
    assert capi.lib().voltrix_abi_version() == 2
    for fn in (voltrix.negative_sample, voltrix.edge_endpoints, voltrix.sample_edge_batch):
        assert callable(fn)
    assert voltrix.EdgeBatch is voltrix.negative.EdgeBatch
    assert (capi.NEGATIVE_MAX_SLOTS, capi.NEGATIVE_MAX_TRIES) == (voltrix.negative.MAX_NEGATIVES, voltrix.negative.MAX_TRIES) == (1024, 256)
    for wrapper in ("launch_negative_sample", "launch_edge_endpoints"):
        assert not hasattr(getattr(capi, wrapper), "timer_label"), wrapper


def test_python_layer_rejects_bad_arguments_before_any_tensor_is_looked_at():
    import torch
    import voltrix

    for k in (0, -1, 1025, 2.0, "4", None, True):
        with pytest.raises(ValueError):
            voltrix.negative_sample(None, None, None, k, 1)
        with pytest.raises(ValueError):
            voltrix.sample_edge_batch(None, None, None, k, (5, 5), 1)
    for tries in (0, -1, 257, 2.0, None, True):
        with pytest.raises(ValueError):
            voltrix.negative_sample(None, None, None, 4, 1, max_tries=tries)
        with pytest.raises(ValueError):
            voltrix.sample_edge_batch(None, None, None, 4, (5, 5), 1, max_tries=tries)
    for seed, offset in ((-1, 0), (2 ** 64, 0), (0, -1), (0, 2 ** 64), (1.5, 0), (0, None)):
        with pytest.raises(ValueError):
            voltrix.negative_sample(None, None, None, 4, seed, offset)
        with pytest.raises(ValueError):
            voltrix.sample_edge_batch(None, None, None, 4, (5, 5), seed, offset)
    for num_cols in (-1, 2 ** 31, 1.5, True):
        with pytest.raises(ValueError):
            voltrix.negative_sample(None, None, None, 4, 1, num_cols=num_cols)
    for fanout in (0, 65, 2.5):
        with pytest.raises(ValueError):
            voltrix.sample_edge_batch(None, None, None, 4, (5, fanout), 1)
    host = torch.zeros(4, dtype=torch.int32)
    wide = torch.zeros(4, dtype=torch.int64)
    for bad in (host, wide, None, [0, 1]):                       # tensors are looked at next: host, int64 or no tensors at all
        with pytest.raises(ValueError):
            voltrix.negative_sample(bad, bad, bad, 4, 1)
        with pytest.raises(ValueError):
            voltrix.edge_endpoints(bad, bad, bad)
        with pytest.raises(ValueError):
            voltrix.sample_edge_batch(bad, bad, bad, 4, (5, 5), 1)


SOURCE = r'''
#include "voltrix/negative_sample_kernels.hpp"
template __global__ void voltrix::negative_sample_kernel<true>(const voltrix::NegativeSampleArgs);
template __global__ void voltrix::negative_sample_kernel<false>(const voltrix::NegativeSampleArgs);
void* the_endpoints() { return reinterpret_cast<void*>(&voltrix::edge_endpoints_kernel); }
'''


def test_every_kernel_compiles_without_scratch_spills_or_lds(tmp_path):
    # the report's remark lines are what profiles/negative_sample/resource_usage.txt holds
    usage, _ = resource_usage(SOURCE, tmp_path, "negative", ("negative_sample_kernel", "edge_endpoints_kernel"))
    # the binary search, the scan and the endpoints: nothing per lane but registers
    assert len(usage) == 3 and len([n for n in usage if "negative_sample_kernel" in n]) == 2, sorted(usage)
    assert all(v == (0, 0, 0, 0) for v in usage.values()), usage
