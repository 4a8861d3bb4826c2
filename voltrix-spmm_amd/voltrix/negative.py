"""Negative sampling on a device CSR, the endpoints of CSR entries and edge mini-batches: what link prediction needs next to
``voltrix.sample_blocks`` (the message-passing layers of any seed set) and ``voltrix.autograd.SDDMM`` (the score of any set of
(row, column) pairs, differentiable in both operands).

    batch = voltrix.sample_edge_batch(indptr, indices, entries, num_negatives=5, fanouts=(10, 25), seed=epoch_seed, offset=step)
    h = encoder(batch.blocks, feat[batch.blocks[0].src_ids])                  # [len(batch.node_ids), D]
    scores = SDDMM(batch.pairs)(h[batch.src_local.long()], h)                 # one score per (source, candidate) pair
    loss = binary_cross_entropy_with_logits(scores, batch.labels)

No reference counterpart.  HIP kernels (voltrix/negative_sample_kernels.hpp) draw, search and reject; torch does the plumbing (range
checks, the count of exhausted slots, prefix sums).  Every result is a function of the arguments alone: the same bits on every run and
on every launch geometry.

THE NEGATIVE RULE (the contract; DESIGN.md 3.25, ``tests/negative_oracle.py`` is the numpy restatement).  ``src``: device int32 ``[S]``
GLOBAL row ids of a CSR ``[num_rows, num_cols]``, duplicates allowed (several positive edges of one source are the normal case).  ``k``
slots per position, ``T = max_tries`` tries per slot, a 64-bit ``seed`` and a 64-bit ``offset``:

* ``draw(p, q)`` is word ``q & 3`` of ``Philox4x32-10(counter = (p, (q >> 2) | 0x40000000, offset & 0xffffffff, offset >> 32),
  key = (seed & 0xffffffff, seed >> 32))``.  ``p`` is the POSITION in ``src``, not the row id: duplicate sources get different
  negatives (the walker index of ``voltrix.random_walk`` does the same).  Bit 30 set with bit 31 clear is the last free domain of counter
  word 1: the dropout mask uses ``00``, the neighbour sampler ``10``, the walk ``11``.  One seed for all four gives unrelated streams.
* Slot ``j`` of position ``p`` uses the draws ``q = j T + t`` for the tries ``t = 0 .. T - 1``.  Try ``t`` proposes
  ``c = (uint64(draw(p, q)) * num_cols) >> 32``; it is rejected if ``c`` occurs in row ``src[p]`` and, with ``exclude_self``, if
  ``c == src[p]``.  ``neg[p, j]`` is the first accepted ``c``, or ``-1`` if all ``T`` tries are rejected (every slot of a full row).
* Slots are independent, so ONE COLUMN MAY APPEAR TWICE in a row of ``neg`` (DGL's uniform sampler behaves the same way).
* ``neg[p, j]`` is a function of ``(seed, offset, p, j, src[p], T, the graph)`` only: not of the launch geometry, of ``k`` or of the
  other sources.  The multiply-shift has a relative bias of at most ``num_cols / 2^32``.
* ``assume_sorted=True`` is the PRECONDITION that every row's columns ascend (duplicates allowed): a binary search, ``O(T log d)`` per
  slot, so a hub row costs only ``log d``.  ``assume_sorted=False`` is a linear scan by the slot's one lane, ``O(T d)``: the slow path,
  not tuned.  On sorted input both give the same bits.
* Entries of ``indices`` outside ``[0, num_cols)`` never match and are never read through.  ``num_cols == 0``: every slot is ``-1``.

ENTRY -> ENDPOINTS.  The package keeps no ``[nnz]`` row-id array, so the row of CSR entry ``e`` is a search: the one ``r`` with
``indptr[r] <= e < indptr[r + 1]``, found as the upper bound of ``e`` in ``indptr`` minus one, which steps over runs of empty rows.

(ROW, COLUMN) -> ENTRY (``find_edges``; DGL's ``edge_ids`` / ``has_edges_between``).  No ``[nnz]`` key array either, so the id of the
FIRST entry of row ``r`` whose column is ``c`` is a search in the row: a lower bound with ``assume_sorted=True`` (the precondition
above), a scan without; ``-1`` where there is none or the row is outside ``[0, num_rows)``.

KEEPING THE BATCH OUT OF ITS BLOCKS.  ``sample_edge_batch(..., exclude_edges="reverse")`` samples the blocks with
``sample_blocks(..., exclude=)``: the batch's own entries and, where ``find_edges(dst, src)`` finds one, the entry of every reverse
``(v, u)``, sorted and deduplicated -- the encoder then aggregates over neither the edge the decoder is asked to predict nor its
reverse (DGL's ``exclude="reverse_id"``).  ``"self"`` leaves out the batch's own entries only.  LIMITATION: in a CSR whose rows hold
duplicate columns only the FIRST reverse entry is excluded.

Host synchronisations: one per ``negative_sample`` (the number of exhausted slots and the "a source is out of range" flag in one
read-back), one per ``edge_endpoints`` ("an entry id is out of range"), none in ``find_edges``, and per ``sample_edge_batch`` the first
two, ``compact_block``'s one (the number of distinct nodes) and ``sample_blocks``' two per layer: ``3 + 2 len(fanouts)`` (plus what the
``CsrPattern`` constructors' transposes cost, as for every ``Block``); with ``exclude_edges`` one more, ``torch.unique``'s (the length
of the exclusion list): ``4 + 2 len(fanouts)``.

Not part of it: degree-weighted negatives; distinct negatives within a row; excluding every duplicate of a
reverse edge.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from .sampling import _INT_MAX, _check_rule_arguments, _device_int32, compact_block, sample_blocks

MAX_NEGATIVES = 1024
MAX_TRIES = 256


def _check_negative_arguments(k, max_tries, seed, offset, num_cols=None) -> None:
    for name, value, top in (("k", k, MAX_NEGATIVES), ("max_tries", max_tries, MAX_TRIES)):
        if isinstance(value, bool) or not isinstance(value, int) or not 1 <= value <= top:
            raise ValueError(f"{name} must be an int in 1..{top}, got {value!r}")
    _check_rule_arguments(None, seed, offset)
    if num_cols is not None and (isinstance(num_cols, bool) or not isinstance(num_cols, int) or not 0 <= num_cols <= _INT_MAX):
        raise ValueError(f"num_cols must be None or an int in [0, 2^31), got {num_cols!r}")


def negative_sample(indptr: torch.Tensor, indices: torch.Tensor, src: torch.Tensor, k: int, seed: int, offset: int = 0,
                    num_cols: int = None, max_tries: int = 16, exclude_self: bool = False, assume_sorted: bool = True):
    """``k`` columns for every position of ``src`` drawn uniformly among those that do not occur in its row, by the module's negative
    rule -> ``(neg, num_exhausted)``: ``neg`` int32 ``[S, k]`` with ``-1`` in every slot whose ``max_tries`` tries were all rejected,
    and the number of such slots.  Every element is written, on the current stream.  DGL's ``negative_sampler.Uniform``, PyG's
    ``structured_negative_sampling``.

    ``indptr`` / ``indices``: a device int32 CSR ``[num_rows, num_cols]``, ``num_cols`` default ``num_rows``; ``src``: device int32
    global row ids, duplicates allowed; views are made contiguous.  ``assume_sorted=True`` requires ascending columns in every row
    (not checked); ``False`` scans each row: the slow path.  ``k`` in 1..1024, ``max_tries`` in 1..256, ``seed`` / ``offset`` in
    ``[0, 2^64)``, ``S k <= INT_MAX``: the scalars are checked before any tensor is looked at.  A source outside ``[0, num_rows)`` is a
    ``ValueError`` from the ONE read-back, which also fetches ``num_exhausted``: the only host synchronisation."""
    from . import capi
    from .jit_kernels.spmm import _raw_stream

    _check_negative_arguments(k, max_tries, seed, offset, num_cols)
    indptr, indices, src = _device_int32(indptr, "indptr"), _device_int32(indices, "indices"), _device_int32(src, "src")
    num_rows = indptr.numel() - 1
    if num_rows < 0:
        raise ValueError("indptr is empty")
    num_cols = num_rows if num_cols is None else num_cols
    dev, count = src.device, src.numel()
    if count * k > _INT_MAX:
        raise ValueError(f"negative_sample: {count} sources of {k} slots; the output is limited to 2^31 - 1 elements")
    neg = torch.empty(count, k, dtype=torch.int32, device=dev)
    if count == 0:
        return neg, 0
    capi.launch_negative_sample(indptr, indices, num_rows, num_cols, src, k, max_tries, exclude_self, assume_sorted, seed, offset, neg,
                                _raw_stream(dev))
    wide = src.long()
    bad, exhausted = torch.stack([((wide < 0) | (wide >= num_rows)).any().long(), (neg < 0).sum()]).tolist()   # the one synchronisation
    if bad:
        raise ValueError(f"negative_sample: a source outside [0, {num_rows})")
    return neg, exhausted


def edge_endpoints(indptr: torch.Tensor, indices: torch.Tensor, entries: torch.Tensor):
    """The endpoints of the CSR entries ``entries`` (device int32 ids in ``[0, nnz)``, any order, duplicates allowed) -> ``(rows, cols)``,
    int32 ``[len(entries)]``: ``rows[i]`` is the row that holds entry ``entries[i]`` -- a search in ``indptr`` by one lane per entry, no
    ``[nnz]`` row-id array -- and ``cols[i] = indices[entries[i]]``.  An id outside ``[0, nnz)`` is a ``ValueError`` from the one
    read-back, the only host synchronisation."""
    from . import capi
    from .jit_kernels.spmm import _raw_stream

    indptr, indices, entries = _device_int32(indptr, "indptr"), _device_int32(indices, "indices"), _device_int32(entries, "entries")
    num_rows = indptr.numel() - 1
    if num_rows < 0:
        raise ValueError("indptr is empty")
    dev, count = entries.device, entries.numel()
    rows = torch.empty(count, dtype=torch.int32, device=dev)
    cols = torch.empty(count, dtype=torch.int32, device=dev)
    if count == 0:
        return rows, cols
    capi.launch_edge_endpoints(indptr, indices, num_rows, entries, rows, cols, _raw_stream(dev))
    if bool((rows < 0).any()):                                                         # the one synchronisation
        raise ValueError(f"edge_endpoints: an entry id outside [0, {indices.numel()})")
    return rows, cols


def find_edges(indptr: torch.Tensor, indices: torch.Tensor, rows: torch.Tensor, cols: torch.Tensor, assume_sorted: bool = True):
    """The CSR entry id of every pair ``(rows[i], cols[i])`` (device int32 ``[Q]`` each, any order, duplicates allowed) -> int32 ``[Q]``:
    the id of the FIRST entry of row ``rows[i]`` whose column is ``cols[i]``, ``-1`` where the row holds no such column or lies outside
    ``[0, num_rows)`` -- so ``find_edges(...) >= 0`` is DGL's ``has_edges_between`` and the ids are its ``edge_ids``.  A search by one
    lane per pair, no ``[nnz]`` key array: ``assume_sorted=True`` requires ascending columns in every row (duplicates allowed; not
    checked) and takes a lower bound, ``O(log d)``; ``False`` scans the row: the slow path.  On sorted rows both give the same bits.
    Every element is written, on the current stream; NO host synchronisation."""
    from . import capi
    from .jit_kernels.spmm import _raw_stream

    indptr, indices = _device_int32(indptr, "indptr"), _device_int32(indices, "indices")
    rows, cols = _device_int32(rows, "rows"), _device_int32(cols, "cols")
    num_rows = indptr.numel() - 1
    if num_rows < 0:
        raise ValueError("indptr is empty")
    if rows.numel() != cols.numel():
        raise ValueError(f"find_edges: {rows.numel()} rows for {cols.numel()} columns")
    out = torch.empty(rows.numel(), dtype=torch.int32, device=rows.device)
    if rows.numel():
        capi.launch_find_edges(indptr, indices, num_rows, rows, cols, assume_sorted, out, _raw_stream(rows.device))
    return out


EXCLUDE_EDGES = (None, "self", "reverse")


@dataclass
class EdgeBatch:
    """A link-prediction mini-batch of ``B`` positive edges.  ``blocks``: the ``Block`` list of ``voltrix.sample_blocks`` whose output
    nodes are ``node_ids`` (``blocks[-1].dst_ids``): an encoder's result has one row per local id.  ``node_ids`` int32: the distinct
    nodes among sources, destinations and negatives, ascending.  ``pairs``: a ``CsrPattern [B, len(node_ids)]`` on LOCAL ids whose row
    ``i`` holds edge ``i``'s destination first, then its non-exhausted negatives in slot order (its transpose is built, so
    ``SDDMM(batch.pairs)`` takes it as it is).  ``labels`` float32 ``[pairs.num_edges]``: 1 for every row's first entry, 0 otherwise.
    ``src_local`` int32 ``[B]``: the local id of every edge's source, so ``x = h[src_local]``.  ``num_exhausted``: the negative slots
    that found no column (absent from ``pairs``)."""
    blocks: list
    node_ids: torch.Tensor
    pairs: object
    labels: torch.Tensor
    src_local: torch.Tensor
    num_exhausted: int


def sample_edge_batch(indptr: torch.Tensor, indices: torch.Tensor, entries: torch.Tensor, num_negatives: int, fanouts, seed: int,
                      offset: int = 0, max_tries: int = 16, exclude_self: bool = True, assume_sorted: bool = True,
                      replace: bool = False, exclude_edges=None) -> EdgeBatch:
    """The mini-batch of the positive edges ``entries`` (device int32 CSR entry ids of a SQUARE CSR) -> ``EdgeBatch``.  Plumbing only:
    ``edge_endpoints``; ``negative_sample(src, num_negatives, seed, offset, ...)`` on the batch's sources; ``compact_block`` without
    seeds for the distinct nodes among sources, destinations and negatives in ascending id (the ``-1`` of an exhausted slot is not an
    id) and everybody's local id; ``sample_blocks(node_ids, fanouts, seed, offset, replace)``; a prefix sum for ``pairs``.  Layer ``l``
    of the blocks is sampled with ``offset + l`` as always; the negatives use ``offset`` itself, and their counter domain keeps them
    apart from layer 0's draws.  ``3 + 2 len(fanouts)`` host synchronisations.

    ``exclude_edges``: ``None`` -- the blocks are sampled from the full graph and hold the batch's positive edges; ``"self"`` -- no
    layer returns one of ``entries``; ``"reverse"`` -- nor the entry ``find_edges(dst, src)`` finds for the reverse ``(v, u)`` of a
    batch edge ``(u, v)`` (a reverse that does not exist is skipped; of duplicate columns only the first entry is found).  The ids are
    sorted and deduplicated with ``torch.unique`` -- one more host synchronisation, ``4 + 2 len(fanouts)`` -- and passed to
    ``sample_blocks(..., exclude=)``.  Any other value is a ``ValueError`` before any tensor is looked at.  The negatives, ``pairs``,
    ``labels``, ``src_local`` and ``node_ids`` do not depend on it; ``exclude_self`` is about the negatives, as before."""
    from .autograd import CsrPattern

    if exclude_edges is not None and not (isinstance(exclude_edges, str) and exclude_edges in EXCLUDE_EDGES):
        raise ValueError(f'exclude_edges must be None, "self" or "reverse", got {exclude_edges!r}')
    _check_negative_arguments(num_negatives, max_tries, seed, offset)
    fanouts = list(fanouts)
    for fanout in fanouts:
        _check_rule_arguments(fanout, seed, offset)
    indptr, indices, entries = _device_int32(indptr, "indptr"), _device_int32(indices, "indices"), _device_int32(entries, "entries")
    num_nodes = indptr.numel() - 1
    src, dst = edge_endpoints(indptr, indices, entries)
    neg, num_exhausted = negative_sample(indptr, indices, src, num_negatives, seed, offset, None, max_tries, exclude_self, assume_sorted)
    dev, count = src.device, src.numel()
    if count == 0:
        raise ValueError("sample_edge_batch: no entries")
    none = torch.empty(0, dtype=torch.int32, device=dev)
    node_ids, local = compact_block(none, torch.cat([src, dst, neg.view(-1)]), num_nodes)
    exclude = None
    if exclude_edges is not None:
        ids = entries
        if exclude_edges == "reverse":
            reverse = find_edges(indptr, indices, dst, src, assume_sorted)
            ids = torch.cat([entries, torch.where(reverse >= 0, reverse, entries)])      # no reverse: the edge itself, once more
        exclude = torch.unique(ids)                           # sorted and distinct: the exclusion rule's precondition
    blocks = sample_blocks(indptr, indices, node_ids, fanouts, seed, offset, replace, exclude)
    src_local = local[:count].contiguous()
    candidates = torch.cat([local[count:2 * count, None], local[2 * count:].view(count, num_negatives)], 1)      # [B, 1 + k], -1: exhausted
    total = candidates.numel() - num_exhausted
    p_indptr = torch.zeros(count + 1, dtype=torch.int32, device=dev)
    if num_exhausted == 0:
        p_indptr[1:] = torch.arange(1, count + 1, dtype=torch.int32, device=dev) * (num_negatives + 1)
        p_indices = candidates.reshape(-1)
    else:                                                     # a stable compaction without a synchronisation: the total is known
        keep = candidates.view(-1) >= 0
        ends = torch.cumsum(keep, 0)
        p_indptr[1:] = ends[num_negatives::num_negatives + 1]
        slots = torch.where(keep, ends - 1, torch.full_like(ends, total))       # the exhausted slots all go to one spare element
        p_indices = torch.empty(total + 1, dtype=torch.int32, device=dev).scatter_(0, slots, candidates.view(-1))[:total].contiguous()
    labels = torch.zeros(total, dtype=torch.float32, device=dev)
    # every row has its positive, so the row starts are distinct entries.  index_fill_ takes the 1 as a launch argument;
    # ``labels[ids] = 1.0`` builds it on the host and copies it over, which is one more host synchronisation
    labels.index_fill_(0, p_indptr[:-1].long(), 1.0)
    pairs = CsrPattern(p_indptr, p_indices, count, node_ids.numel())
    return EdgeBatch(blocks, node_ids, pairs, labels, src_local, num_exhausted)
