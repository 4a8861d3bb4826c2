"""Neighbour sampling on a device CSR and mini-batch blocks for the CSR operators: what produces the rectangular ``[num_dst, num_src]``
patterns that ``spmm_reduce``, ``spmm_heads``, ``attn_aggregate`` and their ``voltrix.autograd`` forms take (GraphSAGE-style training).

    blocks = voltrix.sample_blocks(indptr, indices, batch, fanouts=(10, 25), seed=epoch_seed, offset=step)
    h = feat[blocks[0].src_ids]
    for block, layer in zip(blocks, layers):
        h = layer(SpMMReduce(block.pattern), h)           # h_dst = h[:block.num_dst]: the seeds come first

No reference counterpart.  HIP kernels (voltrix/neighbor_sample_kernels.hpp) select and relabel; torch does the plumbing (degrees,
prefix sums).  The result is a function of the arguments alone -- the same bits on every run, on every launch geometry.

THE SAMPLING RULE (the contract; DESIGN.md 3.23, ``tests/sample_oracle.py`` is the numpy restatement).  For a seed row ``r`` (its
GLOBAL row id), fan-out ``k``, degree ``d = indptr[r + 1] - indptr[r]``, a 64-bit ``seed`` and a 64-bit ``offset``:

* ``draw(r, i)`` is word ``i & 3`` of ``Philox4x32-10(counter = (r, (i >> 2) | 0x80000000, offset & 0xffffffff, offset >> 32),
  key = (seed & 0xffffffff, seed >> 32))``.  Bit 31 of counter word 1 separates these draws from the dropout mask's
  ``(edge, h >> 2, ...)`` counters (``voltrix.dropout_mask``): a model that uses one seed for both gets unrelated streams.
* without replacement, ``d <= k``: every entry of the row, in CSR order; no draw is used.  ``fanout=None`` means this for every row
  (the full neighbourhood, for inference layers), whatever ``replace`` is.
* without replacement, ``d > k``: Floyd's algorithm on entry positions -- for ``i = 0 .. k - 1``, ``j = d - k + i`` and
  ``t = (uint64(draw(r, i)) * (j + 1)) >> 32``; take ``t`` unless it is taken already, then take ``j``.  The ``k`` positions are output
  in ascending order: a sampled row keeps CSR order, sorted rows stay sorted.  A function of ``(seed, offset, r, d, k)`` only: not of
  the other seeds of the batch, their order or the launch geometry.  The multiply-shift has a relative bias of at most ``d / 2^32`` per
  position.
* ``replace=True``, ``d > 0``: exactly ``k`` entries; entry ``i`` is at position ``(uint64(draw(r, i)) * d) >> 32``, in draw order.  A
  row with ``d == 0`` gives none.

THE EXCLUSION RULE (the same contract -- the kernel header states one rule, of which the above is the case ``x = 0``; DESIGN.md 3.26,
``tests/exclude_oracle.py`` is the numpy restatement).  ``exclude`` is a device int32 ``[X]`` of CSR entry ids, STRICTLY ASCENDING
(sorted, distinct), each in ``[0, nnz)``.  For a seed row ``r`` with ``begin = indptr[r]``, ``end = indptr[r + 1]``, ``d = end - begin``:

* ``lo = lower_bound(exclude, begin)``, ``hi = lower_bound(exclude, end)``, ``x = hi - lo``; the excluded positions of the row are
  ``q_i = exclude[lo + i] - begin``, ``i = 0 .. x - 1``, ascending.
* The CANDIDATES are the ``d' = d - x`` positions of the row not among the ``q_i``, in CSR order.  Candidate number ``t`` is position
  ``cand(t) = t + #{i : q_i - i <= t}``; ``q_i - i`` does not decrease, so ``cand(t)`` is one binary search over the row's slice of
  ``exclude``: ``O(log x)``.
* The sampling rule above then applies UNCHANGED WITH ``d'`` IN PLACE OF ``d``, every position it yields mapped through ``cand``:
  ``d' <= k`` without replacement (and ``fanout=None``): every candidate in CSR order; ``d' > k``: Floyd's algorithm on
  ``0 .. d' - 1`` with the same ``draw(r, i)`` and the same counter domain, output ascending; ``replace=True``, ``d' > 0``: ``k``
  entries at ``cand((uint64(draw(r, i)) * d') >> 32)``; ``d' = 0``: nothing.
* So a row none of whose entries is excluded gets exactly the bits it gets without ``exclude``; the result is a function of
  ``(seed, offset, r, d', k)`` and the row's excluded positions only; sorted rows stay sorted; ``s_entries`` still holds ids into the
  original ``indices``.

Cost: one lane per seed, ``O(k^2)`` compares and ``k`` gathers whatever the degree -- a hub row costs what a row of degree ``k + 1``
costs (``fanout=None`` copies a row with one lane: ``O(d)``).  Host synchronisations: one per ``sample_neighbors`` (the total and the
"a seed is out of range" flag in one read-back), one per ``compact_block`` (``num_src``): two per layer of ``sample_blocks``.  With
``exclude`` the kernel adds two binary searches in ``exclude`` per row and one per output entry -- still not a function of the degree --
and the validity of ``exclude`` travels in the same one read-back: no further synchronisation.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

MAX_FANOUT = 64
_INT_MAX = 2 ** 31 - 1


def _check_rule_arguments(fanout, seed, offset) -> None:
    if fanout is not None and (isinstance(fanout, bool) or not isinstance(fanout, int) or not 1 <= fanout <= MAX_FANOUT):
        raise ValueError(f"fanout must be an int in 1..{MAX_FANOUT} or None (every entry), got {fanout!r}")
    for name, value in (("seed", seed), ("offset", offset)):
        if isinstance(value, bool) or not isinstance(value, int) or not 0 <= value < 2 ** 64:
            raise ValueError(f"{name} must be an int in [0, 2^64), got {value!r}")


def _device_int32(t: torch.Tensor, name: str) -> torch.Tensor:
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32 and t.dim() == 1):
        raise ValueError(f"{name} must be a one-dimensional device int32 tensor")
    return t.contiguous()


def sample_neighbors(indptr: torch.Tensor, indices: torch.Tensor, seeds: torch.Tensor, fanout, seed: int, offset: int = 0,
                     replace: bool = False, num_rows: int = None, exclude: torch.Tensor = None):
    """At most ``fanout`` entries of every row in ``seeds``, by the module's sampling rule -> ``(s_indptr, s_indices, s_entries)``: the
    sampled sub-CSR over the seeds (int32 ``[S + 1]``; row ``i`` belongs to ``seeds[i]``), the GLOBAL column id of every sampled entry
    and its CSR entry id in ``indices`` (int32 ``[m]``; for edge features, edge values and ``arg``-style bookkeeping).  Every element
    is written, on the current stream.

    ``indptr`` / ``indices``: device int32 CSR with ``num_rows`` rows (default ``indptr.numel() - 1``); ``seeds``: device int32 global
    row ids, duplicates allowed, any order; views are made contiguous.  ``fanout``: 1..64, or ``None`` for every entry.  The per-seed
    counts and their prefix sum are torch ops; the total ``m`` and an "any seed outside [0, num_rows)" flag come back in ONE small
    read-back, the only host synchronisation.  An out-of-range seed is a ``ValueError``; so are, before any tensor is looked at, a
    ``fanout`` outside 1..64 that is not ``None`` and a ``seed`` or ``offset`` outside ``[0, 2^64)``.

    ``exclude``: ``None`` (the call as it always was), or a device int32 tensor of CSR entry ids, strictly ascending and in
    ``[0, nnz)``, that no row may return: the module's exclusion rule, through the same kernel.  The degrees become ``d'`` by two
    ``torch.searchsorted`` calls; "``exclude`` is not strictly ascending or leaves ``[0, nnz)``" is a third value of the same one
    read-back and a ``ValueError``.  An empty ``exclude`` gives the bits of ``None``; a row without an excluded entry gets them too."""
    from . import capi
    from .jit_kernels.spmm import _raw_stream

    _check_rule_arguments(fanout, seed, offset)
    indptr, indices, seeds = _device_int32(indptr, "indptr"), _device_int32(indices, "indices"), _device_int32(seeds, "seeds")
    if exclude is not None:
        exclude = _device_int32(exclude, "exclude")
        if exclude.numel() == 0:
            exclude = None
    num_rows = indptr.numel() - 1 if num_rows is None else int(num_rows)
    if num_rows < 0 or indptr.numel() != num_rows + 1:
        raise ValueError(f"indptr has {indptr.numel()} elements for {num_rows} rows")
    dev, count = seeds.device, seeds.numel()
    s_indptr = torch.zeros(count + 1, dtype=torch.int32, device=dev)
    if count == 0:
        return s_indptr, torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int32, device=dev)
    if num_rows == 0:
        raise ValueError("sample_neighbors: a seed outside [0, num_rows) (the CSR has no rows)")
    rows = seeds.long()
    bad = (rows < 0) | (rows >= num_rows)
    rows = rows.clamp(0, num_rows - 1)
    degree = torch.where(bad, torch.zeros_like(rows), (indptr[rows + 1] - indptr[rows]).long())
    flags = [bad.any()]                              # what the one read-back carries next to the total
    if exclude is not None:                          # d' = d - x, x = the entries of the row's range that `exclude` holds
        held = torch.searchsorted(exclude, indptr[rows + 1].contiguous()) - torch.searchsorted(exclude, indptr[rows].contiguous())
        degree = torch.where(bad, torch.zeros_like(rows), (degree - held).clamp(min=0))
        flags.append((exclude[1:] <= exclude[:-1]).any() | (exclude[0] < 0) | (exclude[-1] >= indices.numel()))
    if fanout is None:
        taken = degree
    elif replace:
        taken = torch.where(degree > 0, torch.full_like(degree, fanout), torch.zeros_like(degree))
    else:
        taken = degree.clamp(max=fanout)
    ends = torch.cumsum(taken, 0)
    total, any_bad, *any_bad_exclude = torch.stack([ends[-1]] + [flag.long() for flag in flags]).tolist()     # the one synchronisation
    if any(any_bad_exclude):
        raise ValueError(f"sample_neighbors: exclude must be strictly ascending CSR entry ids in [0, {indices.numel()})")
    if any_bad:
        raise ValueError(f"sample_neighbors: a seed outside [0, {num_rows})")
    if total > _INT_MAX:
        raise ValueError(f"sample_neighbors: {total} sampled entries; entry counts are limited to 2^31 - 1")
    s_indptr[1:] = ends
    s_indices = torch.empty(total, dtype=torch.int32, device=dev)
    s_entries = torch.empty(total, dtype=torch.int32, device=dev)
    capi.launch_sample_neighbors(indptr, indices, num_rows, seeds, s_indptr, total, capi.SAMPLE_ALL if fanout is None else fanout,
                                 replace, seed, offset, s_indices, s_entries, _raw_stream(dev), exclude=exclude)
    return s_indptr, s_indices, s_entries


def compact_block(seeds: torch.Tensor, s_indices: torch.Tensor, num_cols: int, validate: bool = False):
    """The source nodes of a sampled block and its columns relabelled -> ``(src_ids, local_indices)``: ``src_ids`` int32 ``[num_src]``
    with ``src_ids[:S] == seeds`` in the given order and ``src_ids[S:]`` the other sampled columns in ascending id (deterministic, and
    ``feat[src_ids]`` gathers ascending addresses); ``local_indices`` int32 ``[m]`` with ``src_ids[local_indices] == s_indices``.

    ``seeds`` (device int32, ids in ``[0, num_cols)``) must not hold duplicates: a precondition, not checked unless ``validate=True``
    (then a ``ValueError``, in the same read-back).  ``s_indices``: device int32 global column ids in ``[0, num_cols)``.  A dense int32
    table of ``num_cols`` entries is cleared, marked by two HIP launches, counted with ``torch.cumsum`` and read by the relabel launch;
    ONE read-back, for ``num_src``."""
    from . import capi
    from .jit_kernels.spmm import _raw_stream

    seeds, s_indices = _device_int32(seeds, "seeds"), _device_int32(s_indices, "s_indices")
    num_cols = int(num_cols)
    if num_cols < 0:
        raise ValueError(f"num_cols must not be negative, got {num_cols}")
    dev, count = seeds.device, seeds.numel()
    stream = _raw_stream(dev)
    if num_cols == 0:
        if count or s_indices.numel():
            raise ValueError("compact_block: ids given for a pattern without columns")
        return torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int32, device=dev)
    table = torch.zeros(num_cols, dtype=torch.int32, device=dev)
    capi.launch_block_mark(s_indices, num_cols, table, stream)
    capi.launch_block_mark_seeds(seeds, num_cols, table, stream)
    rank = torch.cumsum(table > 0, 0, dtype=torch.int32)
    if validate:
        extra, distinct = torch.stack([rank[-1].long(), (table < 0).sum()]).tolist()     # the one synchronisation
        if distinct != count:
            raise ValueError(f"compact_block: {count} seeds, {distinct} distinct ids in [0, {num_cols}) among them")
    else:
        extra = int(rank[-1])                                                            # the one synchronisation
    src_ids = torch.empty(count + extra, dtype=torch.int32, device=dev)
    local = torch.empty(s_indices.numel(), dtype=torch.int32, device=dev)
    capi.launch_block_relabel(s_indices, seeds, table, rank, num_cols, local, src_ids, stream)
    return src_ids, local


@dataclass
class Block:
    """One layer of a mini-batch: ``pattern``, a ``voltrix.autograd.CsrPattern`` ``[num_dst, num_src]`` on the block's LOCAL ids (its
    transpose is built, so every pattern operator takes it as it is); ``src_ids`` int32 ``[num_src]`` and ``dst_ids`` int32
    ``[num_dst]``, the global ids of the local ones, with ``src_ids[:num_dst] == dst_ids`` -- so ``h_dst = h_src[:num_dst]``;
    ``entries`` int32 ``[pattern.num_edges]``, the entry of the sampled graph's CSR that every entry of the pattern is."""
    pattern: object
    src_ids: torch.Tensor
    dst_ids: torch.Tensor
    entries: torch.Tensor
    num_dst: int
    num_src: int


def sample_blocks(indptr: torch.Tensor, indices: torch.Tensor, seeds: torch.Tensor, fanouts, seed: int, offset: int = 0,
                  replace: bool = False, exclude: torch.Tensor = None):
    """The blocks of a ``len(fanouts)``-layer mini-batch whose output nodes are ``seeds`` -> a list of ``Block``, INPUT layer first:
    ``fanouts[i]`` is the fan-out of ``blocks[i]`` (``None``: every neighbour), ``blocks[-1].dst_ids`` is ``seeds`` and the ``dst_ids``
    of every other block are the ``src_ids`` of the block after it.  Layer ``l``, counted from the OUTPUT layer as ``l = 0``, is sampled
    with ``offset + l`` (wrapping at 2^64), so the layers draw from unrelated streams and a caller that steps ``offset`` by
    ``len(fanouts)`` per batch never reuses one.  ``indptr`` / ``indices``: a square device int32 CSR (the sampled columns become the
    next layer's rows); ``seeds``: device int32, no duplicates.  ``exclude`` (``sample_neighbors``' argument: strictly ascending CSR entry
    ids) is left out of EVERY layer.  Two host synchronisations per layer, with or without it."""
    from .autograd import CsrPattern

    fanouts = list(fanouts)
    for fanout in fanouts:
        _check_rule_arguments(fanout, seed, offset)
    indptr, indices, seeds = _device_int32(indptr, "indptr"), _device_int32(indices, "indices"), _device_int32(seeds, "seeds")
    if exclude is not None:
        exclude = _device_int32(exclude, "exclude")
    num_nodes = indptr.numel() - 1
    blocks = []
    dst_ids = seeds
    for layer, fanout in enumerate(reversed(fanouts)):
        s_indptr, s_indices, entries = sample_neighbors(indptr, indices, dst_ids, fanout, seed, (offset + layer) % 2 ** 64, replace,
                                                        num_nodes, exclude)
        src_ids, local = compact_block(dst_ids, s_indices, num_nodes)
        num_dst, num_src = dst_ids.numel(), src_ids.numel()
        blocks.append(Block(CsrPattern(s_indptr, local, num_dst, num_src), src_ids, dst_ids, entries, num_dst, num_src))
        dst_ids = src_ids
    return blocks[::-1]
