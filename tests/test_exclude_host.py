"""CPU: the exclusion rule of the neighbour sampler, the (row, column) -> entry lookup and their plumbing.  A stand-alone
host program runs the headers' own ``exclude_row_count`` / ``exclude_cand`` / ``sample_row`` / ``find_entry`` -- the code the
kernels run -- and agrees with the numpy restatement (tests/exclude_oracle.py): ``cand`` for every row of degree <= 10 and every subset
of excluded positions, the known answers written out here, in the kernel header and in DESIGN.md, uniform draws among the candidates
and never an excluded position; the two entry points are declared, bound and exported; their argument checks are rows of
tests/core_abi_cases.py; the Python layer raises before it looks at a tensor; the lookup kernel, in both instantiations, compiles for gfx950
without scratch, spilled registers or static LDS (the sampling kernel's report is tests/test_sample_host.py's).  No GPU compute is
called here (tests/test_gpu_exclude.py compares the kernels with the same oracle)."""
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO

import exclude_oracle as oracle
import sample_oracle
from kernel_resources import resource_usage
from voltrix import capi

HEADER = os.path.join(REPO, "include", "voltrix_capi.h")
INCLUDE = os.path.join(REPO, "voltrix-spmm_amd", "voltrix", "include")
NAMES = ("voltrix_launch_sample_neighbors_excluding", "voltrix_launch_find_edges")


def _ring():
    """100 nodes, row v = [(v + 1) % 100, (v + 7) % 100, (v + 31) % 100]: not every row ascends."""
    n = 100
    return np.arange(0, 3 * n + 1, 3), np.array([[(v + 1) % n, (v + 7) % n, (v + 31) % n] for v in range(n)]).ravel()


# ---- the rule
RING_EXCLUDE = [0, 15]                  # the first entry of rows 0 and 5
RING_SEEDS = [0, 5, 99, 0, 42]


def test_known_answers_of_the_exclusion_rule():
    """Rows 0 and 5 have d' = 2: with k = 2 they keep their two candidates and use no draw; rows 99 and 42 have d' = 3 and draw as
    they do without ``exclude``."""
    ring = _ring()
    s_indptr, s_indices, s_entries = oracle.sample_neighbors(*ring, RING_SEEDS, 2, 9, 0, False, RING_EXCLUDE)
    assert s_indptr.tolist() == [0, 2, 4, 6, 8, 10]
    assert s_indices.tolist() == [7, 31, 12, 36, 6, 30, 7, 31, 43, 49]
    assert s_entries.tolist() == [1, 2, 16, 17, 298, 299, 1, 2, 126, 127]
    plain = sample_oracle.sample_neighbors(*ring, RING_SEEDS, 2, 9, 0)
    assert np.array_equal(s_entries[4:6], plain[2][4:6]) and np.array_equal(s_entries[8:], plain[2][8:])      # untouched rows
    assert s_entries.dtype == s_indices.dtype == s_indptr.dtype == np.int32
    r_indptr, r_indices, r_entries = oracle.sample_neighbors(*ring, RING_SEEDS, 2, 9, 0, True, RING_EXCLUDE)
    assert r_indptr.tolist() == [0, 2, 4, 6, 8, 10]
    assert r_indices.tolist() == [7, 31, 36, 36, 30, 6, 7, 31, 49, 49]
    assert r_entries.tolist() == [1, 2, 17, 17, 299, 298, 1, 2, 127, 127]
    everything = oracle.sample_neighbors(*ring, RING_SEEDS, None, 9, 0, False, RING_EXCLUDE)
    assert everything[2].tolist() == [1, 2, 16, 17, 297, 298, 299, 1, 2, 126, 127, 128]
    gone = oracle.sample_neighbors(*ring, [0, 1], 2, 9, 0, True, [0, 1, 2, 4])                                # d' = 0, d' = 2
    assert gone[0].tolist() == [0, 0, 2] and gone[2].tolist() == [5, 3]


def test_cand_formula_is_the_definition():
    for degree in range(8):
        for mask in range(1 << degree):
            excluded = [p for p in range(degree) if mask >> p & 1]
            want = oracle.candidates(degree, excluded)
            assert [oracle.cand(excluded, t) for t in range(want.size)] == want.tolist()


# ---- the header's own code in a host program
PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "voltrix/find_edges_kernels.hpp"
#include "voltrix/neighbor_sample_kernels.hpp"

struct ArraySlots {
  std::vector<int> v;
  int get(int j) const { return v.at(j); }
  void set(int j, int x) { v.at(j) = x; }
};

static bool read_ints(const char* path, std::vector<int>& out) {
  std::FILE* f = std::fopen(path, "r");
  if (!f) return false;
  int count = 0;
  if (std::fscanf(f, "%d", &count) != 1) return false;
  out.resize(count);                          // exactly as large as the data: the host's sanitizer sees a read outside it
  for (int& v : out) if (std::fscanf(f, "%d", &v) != 1) return false;
  std::fclose(f);
  return true;
}

// the rule's count for a row with dc candidates
static int rule_count(int dc, int k, bool replace) { return k == INT_MAX ? dc : replace ? (dc > 0 ? k : 0) : (dc < k ? dc : k); }

// argv:
//   "cand" max_degree                                         -> for every d <= max_degree and every subset of excluded positions, one
//                                                                line: x, then cand(t) for t < d - x.  The row begins at entry 1000 + d;
//                                                                the list also holds the entries just before and just after the row
//   "sample" indptr indices exclude replace k seed offset seeds ...   -> one line of entry ids per seed (k = -1: all)
//   "count" indptr indices exclude replace k seed offsets row         -> how often each position of `row` is drawn over offset < offsets
//   "find" indptr indices sorted r c r c ...                          -> one entry id per pair
int main(int argc, char** argv) {
  if (argc < 3) return 2;
  if (!std::strcmp(argv[1], "cand")) {
    const int top = std::atoi(argv[2]);
    for (int d = 0; d <= top; ++d) {
      const int begin = 1000 + d;
      for (int mask = 0; mask < (1 << d); ++mask) {
        std::vector<int> list{begin - 3, begin - 1};
        for (int p = 0; p < d; ++p) if (mask >> p & 1) list.push_back(begin + p);
        list.push_back(begin + d);
        list.push_back(begin + d + 5);
        int first = -1;
        const int x = voltrix::exclude_row_count(list.data(), (int)list.size(), begin, begin + d, &first);
        if (first != 2) return 5;
        std::printf("%d", x);
        for (int t = 0; t < d - x; ++t) std::printf(" %d", voltrix::exclude_cand(list.data() + first, x, begin, t));
        std::printf("\n");
      }
    }
    return 0;
  }
  std::vector<int> indptr, indices, exclude;
  if (argc < 4 || !read_ints(argv[2], indptr) || !read_ints(argv[3], indices)) return 3;
  const int num_rows = (int)indptr.size() - 1;
  if (!std::strcmp(argv[1], "find")) {
    const bool sorted = std::atoi(argv[4]) != 0;
    for (int i = 5; i + 1 < argc; i += 2) {
      const int r = std::atoi(argv[i]), c = std::atoi(argv[i + 1]);
      std::printf("%d\n", sorted ? voltrix::find_entry<true>(indptr.data(), indices.data(), num_rows, r, c)
                                 : voltrix::find_entry<false>(indptr.data(), indices.data(), num_rows, r, c));
    }
    return 0;
  }
  if (argc < 10 || !read_ints(argv[4], exclude)) return 3;
  const bool replace = std::atoi(argv[5]) != 0, counting = !std::strcmp(argv[1], "count");
  const int fanout = std::atoi(argv[6]), k = fanout < 0 ? INT_MAX : fanout;
  const unsigned long long seed = std::strtoull(argv[7], nullptr, 10), last = std::strtoull(argv[8], nullptr, 10);
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  std::vector<long long> hits;
  for (unsigned long long offset = counting ? 0 : last; offset < (counting ? last : last + 1); ++offset) {
    const uint32_t o0 = (uint32_t)offset, o1 = (uint32_t)(offset >> 32);
    for (int i = 9; i < argc; ++i) {
      const int r = std::atoi(argv[i]);
      const int begin = indptr.at(r), d = indptr.at(r + 1) - begin;
      int first = 0;
      const int x = voltrix::exclude_row_count(exclude.data(), (int)exclude.size(), begin, begin + d, &first);
      const int room = rule_count(d - x, k, replace);
      std::vector<int> cols(room), entries(room);   // the row's segment and no more
      ArraySlots slot{std::vector<int>(fanout < 0 ? 0 : fanout, -1)};
      if (d > 0 && room > 0) {
        if (replace)
          voltrix::sample_row<true>(indices.data(), exclude.data(), (int)exclude.size(), (uint32_t)r, begin, d, k, room, k0, k1, o0, o1,
                                    slot, cols.data(), entries.data());
        else
          voltrix::sample_row<false>(indices.data(), exclude.data(), (int)exclude.size(), (uint32_t)r, begin, d, k, room, k0, k1, o0, o1,
                                     slot, cols.data(), entries.data());
      }
      for (int j = 0; j < room; ++j) if (cols[j] != indices.at(entries[j])) return 6;
      if (counting) {
        hits.resize(d, 0);
        for (int j = 0; j < room; ++j) ++hits.at(entries[j] - begin);
      } else {
        for (int j = 0; j < room; ++j) std::printf(j ? " %d" : "%d", entries[j]);
        std::printf("\n");
      }
    }
  }
  for (long long h : hits) std::printf("%lld\n", h);
  return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """The host program, built once: the header as HIP (its kernels are compiled for gfx950 and not launched: the program makes no HIP
    runtime call); the sanitizers are the host's and check the stand-alone program."""
    workdir = tmp_path_factory.mktemp("exclude_host")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src, exe = workdir / "main.hip", workdir / "main"
    src.write_text(PROGRAM)
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", "-Wall", "-Werror", "-Xarch_host", "-fsanitize=address",
                           "-Xarch_host", "-fsanitize=undefined", "-fno-sanitize-recover=all", f"-I{INCLUDE}", str(src), "-o", str(exe)])
    return workdir, str(exe)


def _write(path, values):
    path.write_text(" ".join(str(int(v)) for v in [len(values), *values]))
    return str(path)


def _run(exe, *args):
    return subprocess.run([exe] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout.splitlines()


def test_cand_exhaustively_on_the_host_program(program):
    """Every d <= 10, every subset of excluded positions, every t < d': the header's ``exclude_row_count`` and ``exclude_cand`` against
    the definition (the set difference), with entries of the neighbouring rows in the list on both sides of the row's slice."""
    _, exe = program
    lines = _run(exe, "cand", 10)
    assert len(lines) == 2 ** 11 - 1
    n = values = 0
    for degree in range(11):
        for mask in range(1 << degree):
            excluded = [p for p in range(degree) if mask >> p & 1]
            got = [int(v) for v in lines[n].split()]
            want = oracle.candidates(degree, excluded)
            assert got[0] == len(excluded) and got[1:] == want.tolist(), (degree, excluded)
            assert all(oracle.cand(excluded, t) == want[t] for t in range(want.size))
            n += 1
            values += want.size
    assert values == sum(2 ** d * d // 2 for d in range(11))


def test_host_program_and_oracle_agree_on_the_rule(program):
    workdir, exe = program
    indptr, indices = _ring()
    # a second graph: degrees 0 .. 12 and a row of 200, exclusions at first and last positions, whole rows, runs
    degrees = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 200, 3, 0, 4])
    g_indptr = np.concatenate([[0], np.cumsum(degrees)])
    rng = np.random.default_rng(5)
    g_indices = np.concatenate([np.sort(rng.choice(1000, d, replace=False)) for d in degrees])
    starts = g_indptr[:-1]
    g_exclude = np.unique(np.concatenate([
        [starts[1]], starts[3] + np.arange(3), [starts[4], starts[4] + 3], [starts[5] + 4], [starts[7]], starts[9] + np.arange(2, 7),
        starts[12] + np.array([0, 1, 5, 10, 11]), starts[13] + np.concatenate([np.arange(0, 40), np.arange(90, 200, 3), [199]]),
        [starts[14] + 2], [starts[16]]]))
    files = {"ring": (_write(workdir / "ring_p", indptr), _write(workdir / "ring_i", indices), _write(workdir / "ring_x", RING_EXCLUDE)),
             "mixed": (_write(workdir / "mixed_p", g_indptr), _write(workdir / "mixed_i", g_indices), _write(workdir / "mixed_x", g_exclude)),
             "none": (_write(workdir / "mixed_p", g_indptr), _write(workdir / "mixed_i", g_indices), _write(workdir / "none_x", []))}
    graphs = {"ring": (indptr, indices, RING_EXCLUDE, RING_SEEDS), "mixed": (g_indptr, g_indices, g_exclude, list(range(17)) + [13, 4]),
              "none": (g_indptr, g_indices, [], list(range(17)))}
    rows = 0
    for name, (ip, ix, ex, seeds) in graphs.items():
        for fanout in (1, 2, 3, 5, 64, None):
            for replace in (False, True):
                for seed, offset in ((9, 0), (2 ** 40 + 9, 2 ** 32 + 7)):
                    s_indptr, _, s_entries = oracle.sample_neighbors(ip, ix, seeds, fanout, seed, offset, replace, ex)
                    lines = _run(exe, "sample", *files[name], int(replace), -1 if fanout is None else fanout, seed, offset, *seeds)
                    got = [[int(v) for v in line.split()] for line in lines]
                    want = [s_entries[a:b].tolist() for a, b in zip(s_indptr[:-1], s_indptr[1:])]
                    assert got == want, (name, fanout, replace, seed)
                    assert not set(np.concatenate(got + [[]]).astype(int).tolist()) & set(np.asarray(ex).tolist())
                    if name == "none":             # an empty list: the plain rule's bits
                        assert np.array_equal(s_entries, sample_oracle.sample_neighbors(ip, ix, seeds, fanout, seed, offset, replace)[2])
                    rows += len(seeds)
    assert rows == 24 * (5 + 19 + 17)
    # the known answers, from the header's code
    assert _run(exe, "sample", *files["ring"], 0, 2, 9, 0, *RING_SEEDS) == ["1 2", "16 17", "298 299", "1 2", "126 127"]
    assert _run(exe, "sample", *files["ring"], 1, 2, 9, 0, *RING_SEEDS) == ["1 2", "17 17", "299 298", "1 2", "127 127"]


@pytest.mark.parametrize("replace", [False, True])
def test_every_candidate_is_drawn_equally_and_no_excluded_position_ever(program, replace):
    """One row of degree 16 with 4 excluded positions, k = 3, 40,000 offsets: every candidate's count within 5 sigma of 40000 * 3 / 12
    (binomial sigma without replacement, where a candidate is in a draw with p = 3 / 12; with replacement the count is binomial over
    120,000 draws with p = 1 / 12).  The multiply-shift's bias, at most 12 / 2^32 relative, is orders of magnitude below one sigma."""
    workdir, exe = program
    n, excluded = 40000, [0, 6, 7, 15]                    # the first, a run, the last
    files = (_write(workdir / "u_p", [5, 21]), _write(workdir / "u_i", np.arange(100, 121)), _write(workdir / "u_x", [5 + p for p in excluded]))
    counts = np.array([int(v) for v in _run(exe, "count", *files, int(replace), 3, 20261020, n, 0)])
    assert counts.size == 16 and (counts[excluded] == 0).all() and counts.sum() == 3 * n
    others = np.setdiff1d(np.arange(16), excluded)
    mean = n * 3 / 12
    sigma = (3 * n * (1 / 12) * (11 / 12)) ** 0.5 if replace else (n * 0.25 * 0.75) ** 0.5
    worst = np.abs(counts[others] - mean).max() / sigma
    print(f"worst deviation {worst:.2f} sigma")
    assert others.size == 12 and worst <= 5, (worst, counts.tolist())


def test_find_entry_on_the_host_program(program):
    workdir, exe = program
    degrees = np.array([0, 3, 0, 0, 6, 1, 40, 0])
    indptr = np.concatenate([[0], np.cumsum(degrees)])
    rng = np.random.default_rng(11)
    indices = np.concatenate([np.sort(rng.choice(60, d, replace=False)) for d in degrees])
    indices[indptr[4]:indptr[5]] = [2, 9, 9, 9, 30, 30]                                   # duplicate columns: the first entry wins
    queries = [(r, c) for r in range(-1, 9) for c in (-1, 0, 2, 9, 30, 59, 60)]
    queries += [(r, int(c)) for r in range(8) for c in indices[indptr[r]:indptr[r + 1]]]  # every present pair, first and last included
    rows, cols = [q[0] for q in queries], [q[1] for q in queries]
    want = oracle.find_edges(indptr, indices, rows, cols)
    assert want[queries.index((4, 9))] == indptr[4] + 1 and want[queries.index((4, 30))] == indptr[4] + 4
    assert (want >= 0).sum() >= 50 and (want < 0).sum() >= 50
    flat = [v for q in queries for v in q]
    files = (_write(workdir / "f_p", indptr), _write(workdir / "f_i", indices))
    for is_sorted in (1, 0):
        assert [int(v) for v in _run(exe, "find", *files, is_sorted, *flat)] == want.tolist(), is_sorted
    shuffled = np.concatenate([rng.permutation(indices[a:b]) for a, b in zip(indptr[:-1], indptr[1:])])
    got = [int(v) for v in _run(exe, "find", files[0], _write(workdir / "f_s", shuffled), 0, *flat)]
    assert got == oracle.find_edges(indptr, shuffled, rows, cols).tolist()
    assert [g >= 0 for g in got] == (want >= 0).tolist()


# ---- plumbing
def test_header_declares_and_binding_lists_the_entry_points():
    import voltrix

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in capi.SYMBOLS and name in capi.SIGNATURES, name
        assert hasattr(capi.lib(), name)
    assert capi.lib().voltrix_abi_version() == 2
    assert callable(voltrix.find_edges) and voltrix.find_edges is voltrix.negative.find_edges
    for wrapper in ("launch_sample_neighbors", "launch_find_edges"):       # the one sampling wrapper takes ``exclude=``
        assert callable(getattr(capi, wrapper)) and not hasattr(getattr(capi, wrapper), "timer_label"), wrapper
    assert "exclude" in inspect.signature(capi.launch_sample_neighbors).parameters


def test_python_layer_rejects_bad_arguments_before_any_tensor_is_looked_at():
    import torch
    import voltrix

    for value in ("both", "Reverse", "", 1, True, ("self",), b"self"):
        with pytest.raises(ValueError, match="exclude_edges"):
            voltrix.sample_edge_batch(None, None, None, 4, (5, 5), 1, exclude_edges=value)
    for mode in ("self", "reverse"):                             # the scalars are checked as they always were
        for k in (0, 1025, 2.0, None):
            with pytest.raises(ValueError):
                voltrix.sample_edge_batch(None, None, None, k, (5, 5), 1, exclude_edges=mode)
        for seed, offset in ((-1, 0), (2 ** 64, 0), (0, -1), (0, None)):
            with pytest.raises(ValueError):
                voltrix.sample_edge_batch(None, None, None, 4, (5, 5), seed, offset, exclude_edges=mode)
        with pytest.raises(ValueError):
            voltrix.sample_edge_batch(None, None, None, 4, (5, 65), 1, exclude_edges=mode)
    for fanout in (0, 65, 2.5):
        with pytest.raises(ValueError, match="fanout"):
            voltrix.sample_neighbors(None, None, None, fanout, 1, exclude=None)
        with pytest.raises(ValueError, match="fanout"):
            voltrix.sample_blocks(None, None, None, (5, fanout), 1, exclude=None)
    with pytest.raises(ValueError, match="seed"):
        voltrix.sample_neighbors(None, None, None, 5, -1, exclude=None)
    host = torch.zeros(4, dtype=torch.int32)
    wide = torch.zeros(4, dtype=torch.int64)
    for bad in (host, wide, None, [0, 1]):                       # tensors are looked at next: host, int64 or no tensors at all
        with pytest.raises(ValueError):
            voltrix.find_edges(bad, bad, bad, bad)
        with pytest.raises(ValueError):
            voltrix.sample_neighbors(bad, bad, bad, 5, 1, exclude=host)
        with pytest.raises(ValueError):
            voltrix.sample_blocks(bad, bad, bad, (5, 5), 1, exclude=host)
        with pytest.raises(ValueError):
            voltrix.sample_edge_batch(bad, bad, bad, 4, (5, 5), 1, exclude_edges="reverse")


SOURCE = r'''
#include "voltrix/find_edges_kernels.hpp"
template __global__ void voltrix::find_edges_kernel<true>(const int*, const int*, const int*, const int*, int, int, int*);
template __global__ void voltrix::find_edges_kernel<false>(const int*, const int*, const int*, const int*, int, int, int*);
'''


def test_every_kernel_compiles_without_scratch_spills_or_lds(tmp_path):
    # the report's remark lines are what profiles/sample_exclude/resource_usage.txt holds; the sampling kernel, with and without a
    # list, is tests/test_sample_host.py's
    usage, _ = resource_usage(SOURCE, tmp_path, "exclude", ("find_edges_kernel",))
    # the lower bound and the scan.  The static LDS is 0 (a promoted per-lane array would show here)
    assert len(usage) == 2, sorted(usage)
    assert all(v == (0, 0, 0, 0) for v in usage.values()), usage
