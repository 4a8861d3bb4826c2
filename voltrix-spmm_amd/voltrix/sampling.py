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

THE WEIGHTED RULE (``prob=``; the contract -- voltrix/weighted_sample_kernels.hpp and DESIGN.md 3.27 restate it,
``tests/weighted_sample_oracle.py`` is the numpy restatement).  Integers only: no ``log``, no ``pow`` and no floating-point compare
takes part in a draw, so numpy reproduces every bit.

The table, ``sampling_weights(indptr, prob)``, once per graph.  For an entry ``e`` of row ``r`` with weight ``w_e >= 0`` (finite) and
``m_r`` the row's largest weight, in float64:

* ``q_e = 0`` where ``w_e == 0`` or ``m_r == 0``; otherwise ``q_e = max(1, floor((w_e / m_r) * 2^30))`` -- one correctly rounded
  division, an exact multiplication, an exact floor.  So ``0 <= q_e <= 2^30``, a positive weight stays positive, a zero weight is never
  sampled (DGL's meaning), and ``q_e / 2^30`` is within ``2^-30`` of ``w_e / m_r``.
* ``cum``: int64 ``[nnz]``, the inclusive prefix sum of ``q`` over the whole entry array (at most ``nnz 2^30 < 2^61``); 8 bytes per
  entry.  ``positive``: int32 ``[num_rows]``, the count ``p_r`` of the row's entries with ``q > 0``.

The draw.  Row ``r`` with ``begin = indptr[r]``, ``d = indptr[r + 1] - begin``; ``base = cum[begin - 1]`` (0 for ``begin == 0``),
``c(j) = cum[begin + j] - base``, ``T = c(d - 1)``, ``p = positive[r]``:

* ``draw(r, n)`` is word ``n & 3`` of ``Philox4x32-10(counter = (r, (n >> 2) | 0xA0000000, offset & 0xffffffff, offset >> 32),
  key = (seed & 0xffffffff, seed >> 32))``, ``n < 128``: bits 31 and 29 of counter word 1, a part of the sampling domain the uniform
  rule's draws (``0x80000000 | (i >> 2)``, ``i < 64``) never enter.  ``x_i = (uint64(draw(r, 2 i)) << 32) | draw(r, 2 i + 1)``; a
  uniform integer below ``R`` is ``(x_i R) >> 64``: an entry's probability differs from ``q_e / R`` by less than ``2^-63``.
* without replacement, ``p <= k``: every entry with ``q > 0``, in CSR order; no draw is used.  ``fanout=None`` means this for every row.
* without replacement, ``p > k``: successive sampling -- for ``i = 0 .. k - 1``, ``R_i = T -`` the sum of ``q`` over the entries chosen
  so far, ``t = (x_i R_i) >> 64``; choose the smallest position ``j`` with ``g(j) > t``, ``g(j) = c(j) -`` the sum of ``q_s`` over
  chosen ``s <= j``.  ``g`` does not decrease and is flat at chosen positions and zero weights, so ``j`` is new and has ``q > 0``.  The
  ``k`` positions are output in ascending order: sorted rows stay sorted.
* ``replace=True``, ``T > 0``: exactly ``k`` entries; entry ``i`` is at the smallest ``j`` with ``c(j) > (x_i T) >> 64``, in draw
  order.  ``T == 0``: none.

The result is a function of ``(seed, offset, r, k)`` and the row's ``q`` values only.  EQUAL WEIGHTS DO NOT REPRODUCE THE UNIFORM
RULE'S BITS: another algorithm on another counter domain.  Cost: one lane per seed, ``O(k (k + log d))`` loads of ``cum`` per row
whatever its degree, no loop whose trip count depends on a draw (a row dominated by one weight costs what any row costs); the same one
read-back as the uniform call.  ``prob`` with ``exclude`` is refused: an exclusion list is unbounded per row and would break the
``O(k)`` correction of the removed mass.
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


@dataclass
class SamplingWeights:
    """The integer weight table of the module's weighted rule, built by ``sampling_weights``: ``cum`` int64 ``[nnz]``, the inclusive
    prefix sum of the quantised weights over the whole entry array; ``positive`` int32 ``[num_rows]``, every row's count of entries
    with a positive weight; the host integers ``nnz`` and ``num_rows`` of the CSR it belongs to."""
    cum: torch.Tensor
    positive: torch.Tensor
    nnz: int
    num_rows: int


_PROB_DTYPES = (torch.float32, torch.float64, torch.float16, torch.bfloat16)
_WEIGHT_ONE = float(2 ** 30)


def _quantised_weights(indptr: torch.Tensor, prob: torch.Tensor, num_rows: int):
    """``(q int64 [nnz], invalid)``: the weighted rule's ``q`` and the 0-d flag "a weight is negative or not finite".  Every
    floating-point operation is exact or correctly rounded: the conversion to float64, a maximum, one division, a multiplication by a
    power of two, a floor."""
    w = prob.double()
    nnz = w.numel()
    invalid = (~torch.isfinite(w) | (w < 0)).any()
    # the row of entry e = the rows that end at or before e; clamped, so that an indptr that does not fit prob (refused by the caller's
    # read-back) indexes nothing out of bounds before it is refused
    row_of = torch.searchsorted(indptr[1:].long(), torch.arange(nnz, device=w.device), right=True).clamp(max=num_rows - 1)
    row_max = torch.zeros(num_rows, dtype=torch.float64, device=w.device).scatter_reduce_(0, row_of, w, "amax", include_self=True)
    m = row_max[row_of]
    live = (w > 0) & (m > 0)
    scaled = torch.floor((w / torch.where(live, m, torch.ones_like(m))) * _WEIGHT_ONE)
    q = torch.where(live, scaled.clamp(min=1.0), torch.zeros_like(scaled)).long()
    return q, invalid


def sampling_weights(indptr: torch.Tensor, prob: torch.Tensor) -> SamplingWeights:
    """The weight table of the module's weighted rule for the CSR ``indptr`` and the per-entry weights ``prob`` -> ``SamplingWeights``,
    what ``sample_neighbors(prob=)`` and ``sample_blocks(prob=)`` take.  Built once per graph, torch ops on ``prob``'s device.

    ``indptr``: device int32 ``[num_rows + 1]``; ``prob``: a device tensor ``[nnz]`` of float32, float64, float16 or bfloat16, every
    value finite and ``>= 0`` (anything else is a ``ValueError``; so is ``prob.numel() != indptr[-1]``): the build's single read-back.
    Weights are relative within a row -- ``prob`` and ``c * prob`` give the same table for a power of two ``c`` -- and a zero weight is
    never sampled.  8 bytes per entry."""
    indptr = _device_int32(indptr, "indptr")
    if not (isinstance(prob, torch.Tensor) and prob.is_cuda and prob.dim() == 1 and prob.dtype in _PROB_DTYPES):
        raise ValueError("prob must be a one-dimensional device tensor of float32, float64, float16 or bfloat16")
    if indptr.numel() < 1 or prob.device != indptr.device:
        raise ValueError("indptr must hold num_rows + 1 offsets on prob's device")
    num_rows, nnz = indptr.numel() - 1, prob.numel()
    if num_rows == 0:
        if nnz:
            raise ValueError(f"sampling_weights: prob has {nnz} weights, the CSR no rows")
        dev = prob.device
        return SamplingWeights(torch.empty(0, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int32, device=dev), 0, 0)
    q, invalid = _quantised_weights(indptr, prob, num_rows)
    any_invalid, entries = torch.stack([invalid.long(), indptr[-1].long()]).tolist()          # the one synchronisation
    if entries != nnz:
        raise ValueError(f"sampling_weights: prob has {nnz} weights, the CSR {entries} entries")
    if any_invalid:
        raise ValueError("sampling_weights: every weight must be finite and >= 0")
    cum = torch.cumsum(q, 0)
    ahead = torch.cat([torch.zeros(1, dtype=torch.int64, device=q.device), torch.cumsum(q > 0, 0)])
    positive = (ahead[indptr[1:].long()] - ahead[indptr[:-1].long()]).int()
    return SamplingWeights(cum, positive, nnz, num_rows)


def _check_prob(prob, exclude) -> None:
    if prob is None:
        return
    if not isinstance(prob, SamplingWeights):
        raise ValueError("prob must be the SamplingWeights that voltrix.sampling_weights(indptr, weights) builds, not the weights")
    if exclude is not None:
        raise ValueError("prob together with exclude is not supported (DESIGN.md 3.27)")


def sample_neighbors(indptr: torch.Tensor, indices: torch.Tensor, seeds: torch.Tensor, fanout, seed: int, offset: int = 0,
                     replace: bool = False, num_rows: int = None, exclude: torch.Tensor = None, prob: SamplingWeights = None):
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
    read-back and a ``ValueError``.  An empty ``exclude`` gives the bits of ``None``; a row without an excluded entry gets them too.

    ``prob``: ``None`` (the uniform call as it always was: the same bits, the same kernel), or the ``SamplingWeights`` of this CSR: the
    module's weighted rule, through ``voltrix_sample_neighbors_weighted``.  The per-seed counts come from ``prob.positive`` in place of
    the degrees, inside the same one read-back.  A plain tensor, ``prob`` together with ``exclude`` (both before any tensor is looked
    at) and a table built for another ``nnz`` or ``num_rows`` are a ``ValueError``."""
    from . import capi
    from .jit_kernels.spmm import _raw_stream

    _check_rule_arguments(fanout, seed, offset)
    _check_prob(prob, exclude)
    indptr, indices, seeds = _device_int32(indptr, "indptr"), _device_int32(indices, "indices"), _device_int32(seeds, "seeds")
    if exclude is not None:
        exclude = _device_int32(exclude, "exclude")
        if exclude.numel() == 0:
            exclude = None
    num_rows = indptr.numel() - 1 if num_rows is None else int(num_rows)
    if num_rows < 0 or indptr.numel() != num_rows + 1:
        raise ValueError(f"indptr has {indptr.numel()} elements for {num_rows} rows")
    if prob is not None and (prob.nnz != indices.numel() or prob.num_rows != num_rows):
        raise ValueError(f"sample_neighbors: prob was built for {prob.num_rows} rows and {prob.nnz} entries, the CSR has {num_rows} "
                         f"and {indices.numel()}")
    dev, count = seeds.device, seeds.numel()
    s_indptr = torch.zeros(count + 1, dtype=torch.int32, device=dev)
    if count == 0:
        return s_indptr, torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int32, device=dev)
    if num_rows == 0:
        raise ValueError("sample_neighbors: a seed outside [0, num_rows) (the CSR has no rows)")
    rows = seeds.long()
    bad = (rows < 0) | (rows >= num_rows)
    rows = rows.clamp(0, num_rows - 1)
    if prob is None:
        degree = torch.where(bad, torch.zeros_like(rows), (indptr[rows + 1] - indptr[rows]).long())
    else:                                            # p in place of d: the rule's counts are those of the positive entries (T > 0 iff p > 0)
        degree = torch.where(bad, torch.zeros_like(rows), prob.positive[rows].long())
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
    if prob is not None:
        capi.sample_neighbors_weighted(indptr, indices, prob.cum, num_rows, seeds, s_indptr, total,
                                       capi.SAMPLE_ALL if fanout is None else fanout, replace, seed, offset, s_indices, s_entries,
                                       _raw_stream(dev))
        return s_indptr, s_indices, s_entries
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
                  replace: bool = False, exclude: torch.Tensor = None, prob: SamplingWeights = None):
    """The blocks of a ``len(fanouts)``-layer mini-batch whose output nodes are ``seeds`` -> a list of ``Block``, INPUT layer first:
    ``fanouts[i]`` is the fan-out of ``blocks[i]`` (``None``: every neighbour), ``blocks[-1].dst_ids`` is ``seeds`` and the ``dst_ids``
    of every other block are the ``src_ids`` of the block after it.  Layer ``l``, counted from the OUTPUT layer as ``l = 0``, is sampled
    with ``offset + l`` (wrapping at 2^64), so the layers draw from unrelated streams and a caller that steps ``offset`` by
    ``len(fanouts)`` per batch never reuses one.  ``indptr`` / ``indices``: a square device int32 CSR (the sampled columns become the
    next layer's rows); ``seeds``: device int32, no duplicates.  ``exclude`` (``sample_neighbors``' argument: strictly ascending CSR entry
    ids) is left out of EVERY layer.  Two host synchronisations per layer, with or without it.  ``prob`` (``sample_neighbors``'
    argument: the ``SamplingWeights`` of this CSR) draws every layer by weight -- the graph is square, so one table serves them all;
    ``Block.entries`` still indexes the original CSR, so ``edge_feat[entries]`` works for the weights too.  Not together with
    ``exclude``."""
    from .autograd import CsrPattern

    fanouts = list(fanouts)
    for fanout in fanouts:
        _check_rule_arguments(fanout, seed, offset)
    _check_prob(prob, exclude)
    indptr, indices, seeds = _device_int32(indptr, "indptr"), _device_int32(indices, "indices"), _device_int32(seeds, "seeds")
    if exclude is not None:
        exclude = _device_int32(exclude, "exclude")
    num_nodes = indptr.numel() - 1
    blocks = []
    dst_ids = seeds
    for layer, fanout in enumerate(reversed(fanouts)):
        s_indptr, s_indices, entries = sample_neighbors(indptr, indices, dst_ids, fanout, seed, (offset + layer) % 2 ** 64, replace,
                                                        num_nodes, exclude, prob)
        src_ids, local = compact_block(dst_ids, s_indices, num_nodes)
        num_dst, num_src = dst_ids.numel(), src_ids.numel()
        blocks.append(Block(CsrPattern(s_indptr, local, num_dst, num_src), src_ids, dst_ids, entries, num_dst, num_src))
        dst_ids = src_ids
    return blocks[::-1]
