"""GPU: stream order, host synchronisations and graph capture of the CSR operators that had no such test -- ``sddmm`` (2-D and heads),
``spmm_heads``, ``csr_values_product``, ``spmm_reduce`` / ``spmm_edge`` / ``spmm_rel`` / ``spmm_multi`` with their backwards,
``quantize_fp8`` into ``spmm_fp8``, their autograd wrappers, and the samplers.  The harness and the cases are tests/stream_cases.py.

* delayed producer: the operands' buffers hold NaN (id lists: other in-range ids) until copies enqueued on a side stream BEHIND a
  device-side delay overwrite them; the operator is called on that stream right after the copies.  A launch, cast or pad that is not
  ordered behind the copies reads the prefill and changes the bits.  A control -- the CSR row-gather kernel given the raw handle of a
  second, unrelated side stream -- must change the bits, or the harness sees nothing.
* ``set_sync_debug_mode("error")``: no host read-back where none is promised (the functional operators, ``find_edges`` and a forward
  plus ``backward()`` of every wrapper).
* graph capture that re-reads its inputs: replay, then new values in the static operands, every output poisoned, replay again.
* the host synchronisations the samplers document, counted with ``set_sync_debug_mode("warn")``.

The delay is calibrated once per session (``stream_cases.calibrated_delay``) to at least 20 ms of device time, about three orders of
magnitude above the 25-60 us of host time an eager call costs; 20 ms is a choice, not a measurement.  On the MI355X the calibration gave 71,075,734 cycles of
``torch.cuda._sleep``, measured at 29.8 ms (``test_the_delay_is_long_enough`` prints both, ``-s``); with the delay taken out the control
no longer trips.
"""
import pytest
import torch

import stream_cases as sc

pytestmark = pytest.mark.gpu

SYNC_FREE = sc.names(sync_free=True)
EVERY = sc.names()


def _assert_same(first, second, what):
    assert not sc.differing(first, second), (what, "outputs that differ:", sc.differing(first, second))


@pytest.fixture(scope="module")
def side(cuda_device):
    return torch.cuda.Stream()


# ------------------------------------------------------------------------------------------------------------------ the harness sees
def _row_gather_on(handle):
    """The CSR row-gather sum launched with the raw stream handle ``handle()`` gives, whatever the current stream is."""
    from voltrix import capi

    p = sc.pattern("skewed")

    def run(feat):
        out = torch.empty((p.num_rows, feat.shape[1]), dtype=torch.float32, device="cuda")
        capi.launch_spmm_csr_rows(p.indptr, p.indices, p.num_rows, feat, out, handle(), 1)
        return (out,)

    return run


def test_the_delay_is_long_enough(cuda_device):
    _, kind, count, ms = sc.calibrated_delay()
    print(f"calibrated delay: {count} {kind}, measured {ms:.1f} ms")
    assert ms >= sc.MIN_DELAY_MS


def test_control_a_launch_on_another_stream_changes_the_bits(cuda_device, side):
    """The same procedure with one launch on a second side stream that does not wait for the first: the kernel reads the buffer while
    it still holds the prefill (valid floats: NaN), so the harness must report different bits.  With the right handle it reports none."""
    from voltrix.jit_kernels.spmm import _raw_stream

    p = sc.pattern("skewed")
    feat = sc.randn((p.num_cols, 32), torch.float32, 1)
    other = torch.cuda.Stream()
    right = _row_gather_on(lambda: _raw_stream(feat.device))           # the current stream's handle, as the operators take it
    first = right(feat)
    torch.cuda.synchronize()
    assert not bool(first[0].isnan().any())
    assert sc.differing(first, sc.delayed_producer(right, (feat,), [None], side)) == []
    wrong = sc.delayed_producer(_row_gather_on(lambda: other.cuda_stream), (feat,), [None], side)
    assert sc.differing(first, wrong) == [0], "the control did not trip: the delay is too short for the harness to see a wrong stream"


# ------------------------------------------------------------------------------------------------------------------- delayed producer
@pytest.mark.parametrize("name", EVERY)
def test_delayed_producer(cuda_device, side, name):
    case = sc.get_case(name)
    first = case.eager()
    _assert_same(first, sc.delayed_producer(case.run, case.operands(), case.prefill(), side), name)


@pytest.mark.parametrize("name", SYNC_FREE)
def test_first_agrees_with_the_oracle(cuda_device, name):
    case = sc.get_case(name)
    case.check(case.operands(), case.eager())


def test_late_operands_are_legal(cuda_device):
    """No late operand is an index array of a pattern; every float prefill is NaN and every id prefill another in-range id list."""
    for name in EVERY:
        case = sc.get_case(name)
        structure = set()
        for p in (sc.pattern("skewed"), sc.pattern("rect")):
            structure |= {t.data_ptr() for t in (p.indptr, p.indices, p.t_indptr, p.t_indices, p.t_order, p.etype)}
        for operand, fill in zip(case.operands(), case.prefill()):
            assert operand.data_ptr() not in structure, name
            if fill is None:
                assert operand.dtype.is_floating_point, name
            else:
                n = sc.pattern("skewed").num_rows
                assert fill.dtype == operand.dtype == torch.int32 and fill.shape == operand.shape, name
                assert 0 <= int(fill.min()) and int(fill.max()) < n and 0 <= int(operand.min()) and int(operand.max()) < n, name
                assert not torch.equal(fill, operand), name


# ---------------------------------------------------------------------------------------------------------------- no host read-back
@pytest.mark.parametrize("name", SYNC_FREE)
def test_no_host_read_back(cuda_device, name):
    case = sc.get_case(name)
    first, operands = case.eager(), case.operands()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second = case.run(*operands)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    _assert_same(first, second, name)


# -------------------------------------------------------------------------------------------------------------------- graph capture
@pytest.mark.parametrize("name", SYNC_FREE)
def test_graph_capture_re_reads_its_inputs(cuda_device, name):
    case = sc.get_case(name)
    first, other = case.eager(0), case.eager(1)
    assert sc.differing(first, other), "the second set of values must give other outputs"
    replayed, again = sc.capture_and_replay(case.run, case.operands(0), case.operands(1))
    _assert_same(first, replayed, f"{name}: first replay")
    _assert_same(other, again, f"{name}: replay on new values with poisoned outputs")


# ------------------------------------------------------------------------------------------------- the documented synchronisations
def _counted(monkeypatch, call):
    """``(synchronisations of call() outside the CsrPattern constructors, those inside them)``."""
    import voltrix.autograd

    real = voltrix.autograd.CsrPattern
    inside = [0]
    with sc.SyncCounter() as syncs:
        def counting(*args, **kwargs):
            before = syncs.count()
            made = real(*args, **kwargs)
            inside[0] += syncs.count() - before
            return made

        monkeypatch.setattr(voltrix.autograd, "CsrPattern", counting)
        call()
        total = syncs.count()
    monkeypatch.setattr(voltrix.autograd, "CsrPattern", real)
    torch.cuda.synchronize()
    return total - inside[0], inside[0]


def _sampler_calls():
    """name -> (call, documented synchronisations); fanouts [3, 2] for the formulas."""
    import voltrix
    from voltrix.negative import edge_endpoints, sample_edge_batch
    from voltrix.sampling import compact_block
    from voltrix.subgraph import sample_subgraph_rw, subgraph_csr

    p = sc.pattern("skewed")
    ip, ix, n = p.indptr, p.indices, p.num_rows
    seeds, nodes, sampled = sc.ids(64, n, 500), sc.ids(50, n, 501, distinct=True), sc.ids(200, n, 502)
    entries, columns = sc.ids(40, p.nnz, 503), sc.ids(64, n, 505)        # every input is on the device before anything is counted
    exclude = torch.arange(0, p.nnz, 3, dtype=torch.int32, device="cuda")
    weights = sc.randn((p.nnz,), torch.float32, 504).abs()
    prob = voltrix.sampling_weights(ip, weights)
    fanouts, srt = [3, 2], p.sorted_rows
    return {
        "sample_neighbors": (lambda: voltrix.sample_neighbors(ip, ix, seeds, 3, seed=1), 1),
        "sample_neighbors-exclude": (lambda: voltrix.sample_neighbors(ip, ix, seeds, 3, seed=1, exclude=exclude), 1),
        "sample_neighbors-prob": (lambda: voltrix.sample_neighbors(ip, ix, seeds, 3, seed=1, prob=prob), 1),
        "compact_block": (lambda: compact_block(nodes, sampled, n), 1),
        "compact_block-validate": (lambda: compact_block(nodes, sampled, n, validate=True), 1),
        "subgraph_csr": (lambda: subgraph_csr(ip, ix, nodes), 1),
        "induced_subgraph": (lambda: voltrix.induced_subgraph(ip, ix, nodes), 1),
        "random_walk": (lambda: voltrix.random_walk(ip, ix, seeds, 4, seed=2), 1),
        "negative_sample": (lambda: voltrix.negative_sample(ip, ix, seeds, 4, seed=3, assume_sorted=srt), 1),
        "edge_endpoints": (lambda: edge_endpoints(ip, ix, entries), 1),
        "find_edges": (lambda: voltrix.find_edges(ip, ix, seeds, columns, assume_sorted=srt), 0),
        "sample_blocks": (lambda: voltrix.sample_blocks(ip, ix, nodes, fanouts, seed=4), 2 * len(fanouts)),
        "sample_blocks-exclude": (lambda: voltrix.sample_blocks(ip, ix, nodes, fanouts, seed=4, exclude=exclude), 2 * len(fanouts)),
        "sample_edge_batch": (lambda: sample_edge_batch(ip, ix, entries, 3, fanouts, seed=5, assume_sorted=srt), 3 + 2 * len(fanouts)),
        "sample_edge_batch-reverse": (lambda: sample_edge_batch(ip, ix, entries, 3, fanouts, seed=5, assume_sorted=srt,
                                                                exclude_edges="reverse"), 4 + 2 * len(fanouts)),
        "sample_subgraph_rw": (lambda: sample_subgraph_rw(ip, ix, seeds, 4, seed=6), 3),
        "sampling_weights": (lambda: voltrix.sampling_weights(ip, weights), 1),
    }


SAMPLER_CALLS = ("sample_neighbors", "sample_neighbors-exclude", "sample_neighbors-prob", "compact_block", "compact_block-validate",
                 "subgraph_csr", "induced_subgraph", "random_walk", "negative_sample", "edge_endpoints", "find_edges", "sample_blocks",
                 "sample_blocks-exclude", "sample_edge_batch", "sample_edge_batch-reverse", "sample_subgraph_rw", "sampling_weights")


def test_control_two_reads_count_as_two(cuda_device, monkeypatch):
    x = torch.arange(4, device="cuda")

    def two_reads():
        return x[1].item() + x[2].item()

    assert _counted(monkeypatch, two_reads) == (2, 0)
    assert _counted(monkeypatch, lambda: x + 1) == (0, 0)


@pytest.mark.parametrize("name", SAMPLER_CALLS)
def test_documented_synchronisations(cuda_device, monkeypatch, name):
    """The counts the docstrings of sampling.py, subgraph.py and negative.py give; what the ``CsrPattern`` constructors cost is counted
    apart, as the docstrings say."""
    calls = _sampler_calls()
    assert tuple(calls) == SAMPLER_CALLS
    call, documented = calls[name]
    call()                                             # the first call loads the kernels
    torch.cuda.synchronize()
    counted, in_patterns = _counted(monkeypatch, call)
    print(f"{name}: {counted} host synchronisations of its own (documented {documented}), {in_patterns} in CsrPattern constructors")
    assert counted == documented, (name, counted, documented, in_patterns)
