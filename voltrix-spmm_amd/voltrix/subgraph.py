"""Induced subgraphs and random walks on a device CSR: subgraph mini-batch training (Cluster-GCN: a batch is a cluster; GraphSAINT-RW:
a batch is the nodes a set of random walks visits).  The sibling of ``voltrix.sampling`` (node-wise mini-batches).

    sub = voltrix.induced_subgraph(indptr, indices, nodes)                    # Subgraph(pattern [S, S], node_ids, entries, num_nodes)
    h = layer(SpMMReduce(sub.pattern, reduce="mean"), feat[sub.node_ids])     # every pattern operator takes sub.pattern as it is
    sub = voltrix.sample_subgraph_rw(indptr, indices, roots, length=4, seed=epoch_seed, offset=step)

No reference counterpart.  HIP kernels (voltrix/induced_subgraph_kernels.hpp) count, compact and walk; torch does the plumbing (the
table's clear, prefix sums, the range checks).  Every result is a function of the arguments alone: the same bits on every run, on
every launch geometry, for every lane-group width.

THE SUBGRAPH CONTRACT (``tests/subgraph_oracle.py`` is the numpy restatement).  ``rows``: device int32 ``[R]`` global
row ids, any order, duplicates allowed (a duplicate row is emitted twice).  ``cols``: device int32 ``[C]`` global column ids in
``[0, num_cols)``, NO duplicates; default ``rows`` -- then the result is square and ``rows`` must itself be free of duplicates.
``num_cols`` defaults to ``indptr.numel() - 1``.

* Row ``i`` of the result is row ``rows[i]`` of the CSR with exactly those entries whose column is in ``cols``, IN CSR ORDER: a stable
  compaction.  A sorted row stays sorted only if ``cols`` is ascending.  A column that appears twice in a row is kept twice.
* ``s_local[e]`` is the position in ``cols`` of the entry's column: the local id of ``cols[j]`` is ``j``, so ``feat[cols]`` is the
  subgraph's feature matrix.  ``s_entries[e]`` is the entry's index in ``indices`` (edge values, edge features, ``arg``-style
  bookkeeping): the meaning it has in ``sample_neighbors``.
* Columns in ``indices`` outside ``[0, num_cols)`` are never selected and never read through.
* A row id outside ``[0, num_rows)`` is a ``ValueError``, so is a ``cols`` id outside ``[0, num_cols)`` and, with ``validate=True``, a
  duplicate in ``cols``.  All of these come back in the ONE read-back that also fetches the total: the only host synchronisation of
  ``subgraph_csr``.  Totals above ``INT_MAX`` are refused.
* Every element of the three outputs is written; nothing needs initialising.  No atomics.

Mechanism: a dense int32 table of ``num_cols`` entries, cleared and marked ``table[cols[j]] = -(j + 1)`` by the marker
``compact_block`` uses; a count launch (a lane group of 4 / 8 / 16 / 32 / 64 lanes per row, chosen from the graph's mean degree), a
``torch.cumsum``, the read-back, and a fill launch: the same walk, a stable compaction through the group's slice of a wave's ballot.
A hub row is walked by one group: the row-per-group weakness DESIGN 3.10 / 3.13 name.

THE WALK RULE.  ``nodes[w, 0] = starts[w]``.  At step ``t`` (0-based) walker ``w`` stands on node ``v`` of degree ``d``:

* ``d == 0``: the walk is over; this and every later step write ``-1`` in ``nodes`` and in ``entries``.
* otherwise the walker takes the entry at position ``(uint64(draw(w, t)) * d) >> 32`` of row ``v``: ``entries[w, t]`` is its CSR entry
  id, ``nodes[w, t + 1]`` its column.
* ``draw(w, t)`` is word ``t & 3`` of ``Philox4x32-10(counter = (w, (t >> 2) | 0xC0000000, offset & 0xffffffff, offset >> 32),
  key = (seed & 0xffffffff, seed >> 32))``.  Bits 31 AND 30 of counter word 1 separate these draws from the neighbour sampler's
  (``(i >> 2) | 0x80000000``, ``i < 64``) and from the dropout mask's (``h >> 2 < 2^29``): one seed for all three gives unrelated
  streams.
* A column id outside ``[0, num_rows)`` (a rectangular CSR) is recorded as it is and ends the walk like a dead end: never an
  out-of-bounds read of ``indptr``.
* ``w`` is the walker's index in ``starts``: duplicate starts are different walks.  The result is a function of ``(seed, offset, w,
  starts[w], the graph)`` only, not of the launch geometry.

Host synchronisations: one per ``subgraph_csr`` / ``induced_subgraph`` (plus what the ``CsrPattern`` constructor's transpose costs
every ``Block`` as well), one per ``random_walk`` (the "a start is out of range" flag), three per ``sample_subgraph_rw``: the walk's,
``compact_block``'s (the number of distinct nodes) and ``subgraph_csr``'s.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from .sampling import _INT_MAX, _check_rule_arguments, _device_int32, compact_block

MAX_WALK_LENGTH = 2 ** 20
GROUPS = (4, 8, 16, 32, 64)


def group_for(num_entries: int, num_rows: int) -> int:
    """The lane-group width for a graph of this mean degree: the smallest width that covers a mean row in one round.  Known on the host
    without a synchronisation; DESIGN.md 3.24 has the measurement behind it."""
    mean = num_entries / max(1, num_rows)
    for group in GROUPS:
        if mean <= group:
            return group
    return GROUPS[-1]


def _check_length(length) -> None:
    if isinstance(length, bool) or not isinstance(length, int) or not 0 <= length <= MAX_WALK_LENGTH:
        raise ValueError(f"length must be an int in [0, 2^20], got {length!r}")


def subgraph_csr(indptr: torch.Tensor, indices: torch.Tensor, rows: torch.Tensor, cols: torch.Tensor = None, num_cols: int = None,
                 validate: bool = False, group: int = None):
    """Rows ``rows`` of a device int32 CSR restricted to the columns ``cols`` -> ``(s_indptr, s_local, s_entries)``: int32 ``[R + 1]``,
    and for every kept entry, in CSR order, the position of its column in ``cols`` and its index in ``indices`` (int32 ``[m]``); the
    module's subgraph contract.  ``cols=None``: ``rows`` (a square result; ``rows`` without duplicates).  ``group``: the lane-group
    width (4 / 8 / 16 / 32 / 64), default from the mean degree; every width gives the same bits.  Views are made contiguous.  ONE
    read-back: the total, "a row is out of range", "a column id is out of range" and, with ``validate``, the number of distinct ids
    in ``cols``; each of the last three a ``ValueError``."""
    from . import capi
    from .jit_kernels.spmm import _raw_stream

    indptr, indices, rows = _device_int32(indptr, "indptr"), _device_int32(indices, "indices"), _device_int32(rows, "rows")
    cols = rows if cols is None else _device_int32(cols, "cols")
    num_rows = indptr.numel() - 1
    if num_rows < 0:
        raise ValueError("indptr is empty")
    num_cols = num_rows if num_cols is None else int(num_cols)
    if num_cols < 0:
        raise ValueError(f"num_cols must not be negative, got {num_cols}")
    group = group_for(indices.numel(), num_rows) if group is None else group
    if group not in GROUPS:
        raise ValueError(f"group must be one of {GROUPS}, got {group!r}")
    dev, count = rows.device, rows.numel()
    stream = _raw_stream(dev)
    s_indptr = torch.zeros(count + 1, dtype=torch.int32, device=dev)
    table = torch.zeros(max(num_cols, 1), dtype=torch.int32, device=dev)
    capi.launch_block_mark_seeds(cols, num_cols, table[:num_cols], stream)
    counts = torch.empty(count, dtype=torch.int32, device=dev)
    if count and indices.numel():
        capi.launch_subgraph_count(indptr, indices, num_rows, rows, table[:num_cols], group, counts, stream)
    else:
        counts.zero_()
    ends = torch.cumsum(counts, 0, dtype=torch.int64)
    wide_rows, wide_cols = rows.long(), cols.long()
    flags = [ends[-1] if count else torch.zeros((), dtype=torch.int64, device=dev),
             ((wide_rows < 0) | (wide_rows >= num_rows)).any().long(), ((wide_cols < 0) | (wide_cols >= num_cols)).any().long()]
    if validate:
        flags.append((table < 0).sum())
    total, bad_row, bad_col, *distinct = torch.stack(flags).tolist()                    # the one synchronisation
    if bad_row:
        raise ValueError(f"subgraph_csr: a row outside [0, {num_rows})")
    if bad_col:
        raise ValueError(f"subgraph_csr: a column id outside [0, {num_cols})")
    if validate and distinct[0] != cols.numel():
        raise ValueError(f"subgraph_csr: {cols.numel()} column ids, {distinct[0]} distinct among them")
    if total > _INT_MAX:
        raise ValueError(f"subgraph_csr: {total} kept entries; entry counts are limited to 2^31 - 1")
    s_indptr[1:] = ends
    s_local = torch.empty(total, dtype=torch.int32, device=dev)
    s_entries = torch.empty(total, dtype=torch.int32, device=dev)
    if total:
        capi.launch_subgraph_fill(indptr, indices, num_rows, rows, table[:num_cols], group, s_indptr, s_local, s_entries, stream)
    return s_indptr, s_local, s_entries


@dataclass
class Subgraph:
    """A graph restricted to ``num_nodes`` of its nodes: ``pattern``, a ``voltrix.autograd.CsrPattern`` ``[num_nodes, num_nodes]`` on
    LOCAL ids (its transpose is built, so every pattern operator takes it as it is); ``node_ids`` int32 ``[num_nodes]``, the global id
    of every local one (``feat[node_ids]`` is the subgraph's feature matrix); ``entries`` int32 ``[pattern.num_edges]``, the entry of
    the graph's CSR that every entry of the pattern is."""
    pattern: object
    node_ids: torch.Tensor
    entries: torch.Tensor
    num_nodes: int


def induced_subgraph(indptr: torch.Tensor, indices: torch.Tensor, nodes: torch.Tensor, validate: bool = False) -> Subgraph:
    """The square device int32 CSR restricted to ``nodes`` (device int32, no duplicates, any order; local id ``j`` is ``nodes[j]``) ->
    ``Subgraph``: ``subgraph_csr(rows=nodes, cols=nodes)`` as a ``CsrPattern [S, S]``.  DGL's ``node_subgraph``, PyG's ``subgraph``.
    One read-back of its own; the transpose is built by the kernels every ``CsrPattern`` uses."""
    from .autograd import CsrPattern

    nodes = _device_int32(nodes, "nodes")
    s_indptr, s_local, entries = subgraph_csr(indptr, indices, nodes, None, None, validate)
    count = nodes.numel()
    return Subgraph(CsrPattern(s_indptr, s_local, count, count), nodes, entries, count)


def random_walk(indptr: torch.Tensor, indices: torch.Tensor, starts: torch.Tensor, length: int, seed: int, offset: int = 0):
    """``W = starts.numel()`` uniform random walks of ``length`` steps by the module's walk rule -> ``(nodes, entries)``: int32
    ``[W, length + 1]`` (``nodes[:, 0]`` is ``starts``) and int32 ``[W, length]``, the CSR entry taken at every step; ``-1`` in both
    once a walk has met a node without entries.  Every element is written, on the current stream.

    ``starts``: device int32 in ``[0, num_rows)``, duplicates allowed (different walks); anything else is a ``ValueError`` from the
    one read-back that is this function's only synchronisation.  ``length``: an int in ``[0, 2^20]`` with ``W (length + 1) <= INT_MAX``;
    ``seed`` / ``offset``: ints in ``[0, 2^64)``; all three are checked before any tensor is looked at."""
    from . import capi
    from .jit_kernels.spmm import _raw_stream

    _check_length(length)
    _check_rule_arguments(None, seed, offset)
    indptr, indices, starts = _device_int32(indptr, "indptr"), _device_int32(indices, "indices"), _device_int32(starts, "starts")
    num_rows = indptr.numel() - 1
    if num_rows < 0:
        raise ValueError("indptr is empty")
    dev, count = starts.device, starts.numel()
    if count * (length + 1) > _INT_MAX:
        raise ValueError(f"random_walk: {count} walkers of {length + 1} nodes; the outputs are limited to 2^31 - 1 elements")
    nodes = torch.empty(count, length + 1, dtype=torch.int32, device=dev)
    entries = torch.empty(count, length, dtype=torch.int32, device=dev)
    if count == 0:
        return nodes, entries
    capi.launch_random_walk(indptr, indices, num_rows, starts, length, seed, offset, nodes, entries, _raw_stream(dev))
    wide = starts.long()
    if bool(((wide < 0) | (wide >= num_rows)).any()):                                  # the one synchronisation
        raise ValueError(f"random_walk: a start outside [0, {num_rows})")
    return nodes, entries


def sample_subgraph_rw(indptr: torch.Tensor, indices: torch.Tensor, roots: torch.Tensor, length: int, seed: int,
                       offset: int = 0) -> Subgraph:
    """GraphSAINT's random-walk node sampler: the square graph restricted to the distinct nodes that ``random_walk(roots, length, seed,
    offset)`` visits, in ascending id -> ``Subgraph``.  Plumbing only: the walk, ``compact_block`` without seeds (the distinct marked
    ids ascending; the ``-1`` padding is not an id) and ``induced_subgraph``.  Three host synchronisations, one per part.  GraphSAINT's
    normalisation coefficients are not part of it."""
    nodes, _ = random_walk(indptr, indices, roots, length, seed, offset)
    none = torch.empty(0, dtype=torch.int32, device=nodes.device)
    visited, _ = compact_block(none, nodes.view(-1), indptr.numel() - 1)
    return induced_subgraph(indptr, indices, visited)
