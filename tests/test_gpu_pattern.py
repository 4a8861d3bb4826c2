"""One ``CsrPattern`` shared by the five attention operators gives what five operators built from the raw CSR give: the same kernels on
the same inputs, so forward outputs and every input gradient are equal bit for bit; nothing of the pattern is copied or built again."""
import pytest
import torch

pytestmark = pytest.mark.gpu

NUM_ROWS, NUM_COLS, HEADS, DIM = 70, 50, 3, 8
OPERATORS = ("SDDMM", "SpMMHeads", "GATScore", "GATv2Score", "AttnAggregate")


def _csr():
    """70 x 50, row 5 empty, entry (0, 3) twice, column 7 in a quarter of the entries."""
    g = torch.Generator().manual_seed(7)
    rows = []
    for r in range(NUM_ROWS):
        if r == 5:
            rows.append([])
            continue
        cols = torch.randperm(NUM_COLS - 1, generator=g)[:3].tolist()
        cols = sorted(c if c < 7 else c + 1 for c in cols)        # three columns that are not 7 ...
        rows.append(cols + [7])                                    # ... and column 7: one entry in four
    rows[0] = sorted([3, 3, 7] + [c for c in rows[0] if c not in (3, 7)][:1])      # a duplicated edge
    indptr = torch.tensor([0] + [len(r) for r in rows]).cumsum(0).to(torch.int32)
    indices = torch.tensor([c for r in rows for c in r], dtype=torch.int32)
    nnz = indices.numel()
    assert int((indices == 7).sum()) * 4 == nnz and indptr[5] == indptr[6]
    return indptr.cuda(), indices.cuda()


@pytest.fixture(scope="module")
def graph(cuda_device):
    return _csr()


def _inputs(name, nnz, dtype):
    """The operator's inputs, node tensors in ``dtype`` and edge tensors in float32."""
    g = torch.Generator().manual_seed(11)

    def node(n, *shape):
        return torch.randn(n, *shape, generator=g).to(dtype).cuda()

    edge = torch.randn(nnz, HEADS, generator=g).cuda()
    return {"SDDMM": lambda: (node(NUM_ROWS, HEADS, DIM), node(NUM_COLS, HEADS, DIM)),
            "SpMMHeads": lambda: (node(NUM_COLS, HEADS, DIM), edge),
            "GATScore": lambda: (node(NUM_ROWS, HEADS), node(NUM_COLS, HEADS)),
            "GATv2Score": lambda: (node(NUM_ROWS, HEADS, DIM), node(NUM_COLS, HEADS, DIM), torch.randn(HEADS, DIM, generator=g).cuda()),
            "AttnAggregate": lambda: (node(NUM_COLS, HEADS, DIM), edge)}[name]()


def _run(op, inputs):
    """Forward output and the gradient of every input, for a fixed upstream gradient."""
    leaves = [t.clone().requires_grad_() for t in inputs]
    out = op(*leaves)
    upstream = torch.randn(out.shape, generator=torch.Generator().manual_seed(13)).cuda()
    out.backward(upstream)
    return [out.detach()] + [t.grad for t in leaves]


@pytest.mark.parametrize("dtype", (torch.float32, torch.float16), ids=("fp32", "fp16"))
def test_a_shared_pattern_gives_the_bits_of_five_patterns(graph, dtype):
    from voltrix import autograd

    indptr, indices = graph
    pattern = autograd.CsrPattern(indptr, indices, NUM_ROWS, NUM_COLS)
    assert pattern.t_order.dtype == torch.int32 and pattern.num_edges == indices.numel()
    for name in OPERATORS:
        cls = getattr(autograd, name)
        own, shared = cls(indptr, indices, NUM_ROWS, NUM_COLS), cls(pattern)
        assert shared.pattern is pattern and shared.t_indptr is pattern.t_indptr and shared.t_indices is pattern.t_indices
        assert shared.t_order is pattern.t_order and shared.indptr is pattern.indptr and shared.indices is pattern.indices
        assert own.t_order.dtype == torch.int32 and shared.t_order.dtype == torch.int32
        assert (own.num_rows, own.num_cols, own.num_edges) == (NUM_ROWS, NUM_COLS, indices.numel())
        assert torch.equal(own.t_indptr, pattern.t_indptr) and torch.equal(own.t_order, pattern.t_order)
        with pytest.raises(AttributeError):
            shared.t_order = None                       # read-only
        inputs = _inputs(name, indices.numel(), dtype)
        for a, b in zip(_run(own, inputs), _run(shared, inputs)):
            assert a.dtype == b.dtype and torch.equal(a, b), name


def test_transposed_tuple_with_an_int64_order_is_converted(graph):
    from voltrix import autograd

    indptr, indices = graph
    pattern = autograd.CsrPattern(indptr, indices, NUM_ROWS, NUM_COLS)
    given = (pattern.t_indptr, pattern.t_indices, pattern.t_order.long())
    for name in OPERATORS:
        op = getattr(autograd, name)(indptr, indices, NUM_ROWS, NUM_COLS, transposed=given)
        assert op.t_indptr is pattern.t_indptr and op.t_indices is pattern.t_indices
        assert op.t_order.dtype == torch.int32 and torch.equal(op.t_order, pattern.t_order)
        inputs = _inputs(name, indices.numel(), torch.float32)
        for a, b in zip(_run(op, inputs), _run(getattr(autograd, name)(pattern), inputs)):
            assert torch.equal(a, b), name
    with pytest.raises(AssertionError):                 # the size checks of the tuple stay
        autograd.CsrPattern(indptr, indices, NUM_ROWS, NUM_COLS, transposed=(pattern.t_indptr[:-1], pattern.t_indices, pattern.t_order))


@pytest.mark.parametrize("name", ("SDDMM", "SpMMHeads"))
def test_int32_order_selects_what_the_int64_order_selected(graph, name):
    """``g[t_order]`` in the backward of ``SDDMM`` / ``SpMMHeads``: the operators kept an int64 order before."""
    from voltrix import autograd

    indptr, indices = graph
    op = getattr(autograd, name)(indptr, indices, NUM_ROWS, NUM_COLS)
    inputs = _inputs(name, indices.numel(), torch.float32)
    got = _run(op, inputs)
    op.pattern.t_order = op.pattern.t_order.long()
    assert op.t_order.dtype == torch.int64
    for a, b in zip(got, _run(op, inputs)):
        assert torch.equal(a, b)
