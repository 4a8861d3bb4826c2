"""GPU: the ticket join as the DEFAULT of every public two-level path, with the mode asserted.

Nothing here names a join: what runs is what ``hybrid.join_mode`` picks.  The first call on a handle chooses the window kernel's tile
and still takes the atomic join; from the second call on the step is a ticket step, and ``hybrid.LAST_JOIN`` has to say so.  Covered:
``spmm_two_level`` on an explicit handle (512-row panels, tau = 24: the graph of test_gpu_ticket_join.py at N = 1033, a partial last
block) and ``voltrix.spmm`` on a ``csr_preprocess`` handle with its side-car (at the default tau the panel side dominates this graph,
so the side-car has 256-row panels and the pipelined panel kernel); fp16, bf16, a padded width and fp32 features with a scale that is
not 1; poisoned scratch; HIP-graph replays (the tickets have to be zeroed INSIDE the graph); two user streams; autograd."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import voltrix
from oracle import oracle_np
from poisoned_alloc import poisoned
from test_gpu_spmm import _assert_close
from test_gpu_ticket_join import _build, _graph
from voltrix import hybrid, sidecar
from voltrix.graphed import GraphedSpMM
from voltrix.jit_kernels.spmm import handle_unit_table
from voltrix.spmm.spmm import _operand

pytestmark = pytest.mark.gpu

N = 1033


@pytest.fixture(autouse=True)
def _untuned_pair(monkeypatch):
    monkeypatch.setenv("VOLTRIX_TUNE_SPACE", "none")
    monkeypatch.setenv("VOLTRIX_FUSED", "0")


def _explicit(tag, name="hub"):
    """(indptr, indices, call): ``spmm_two_level`` on a new explicit handle."""
    indptr, indices, two = _build(name, N, 4, tag=tag)
    return indptr, indices, two, lambda feat: voltrix.spmm_two_level(two, feat)


def _side_car(tag, monkeypatch):
    """(indptr, indices, side-car, call, handle): ``voltrix.spmm`` on a ``csr_preprocess`` handle whose side-car is attached."""
    monkeypatch.setenv("VOLTRIX_HYBRID", "1")
    monkeypatch.setenv("VOLTRIX_HYBRID_MIN_SHARE", "0")
    indptr, indices = _graph(True, N)
    handle = voltrix.csr_preprocess(torch.from_numpy(indptr), torch.from_numpy(indices), N)
    handle[1].hash_tag = tag
    known, two, csr = sidecar.lookup_both(handle[1])
    assert known and isinstance(two, voltrix.TwoLevelHandle) and csr is None
    plan = two.plan
    assert plan.num_ksteps > 0 and plan.num_shared_edges > 0 and plan.num_resid_edges > 0
    assert (plan.waves, plan.row_blocks) == (8, hybrid.PANEL_DOMINATED_ROW_BLOCKS)      # 256-row panels: the pipelined panel kernel
    assert hybrid.default_panel_tile(128, plan.waves, plan.row_blocks)[2] == hybrid.KSTEPS_PIPELINED
    return indptr, indices, two, lambda feat: voltrix.spmm(*handle, num_nodes=N, num_edges=len(indices), feat=feat), handle


def _entry(entry, tag, monkeypatch):
    return _explicit(tag) if entry == "spmm_two_level" else _side_car(tag, monkeypatch)[:4]


def _call_with_mode(call, feat, want):
    hybrid.LAST_JOIN["mode"] = hybrid.LAST_JOIN["tickets"] = None
    out = call(feat)
    assert hybrid.LAST_JOIN["mode"] == want, (hybrid.LAST_JOIN["mode"], want)
    assert (hybrid.LAST_JOIN["tickets"] is not None) == (want == "ticket")
    return out


KINDS = {"fp16-F128": (torch.float16, 128, "fp16"), "bf16-F64": (torch.bfloat16, 64, "exact"), "fp16-F100": (torch.float16, 100, "fp16"),
         "fp32-scaled-F128": (torch.float32, 128, "fp16-scaled")}


@pytest.mark.parametrize("entry", ["spmm_two_level", "spmm"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_first_call_atomic_then_ticket(cuda_device, kind, entry, monkeypatch):
    dtype, f, mode = KINDS[kind]
    indptr, indices, two, call = _entry(entry, f"ticket_paths_{entry}_{kind}", monkeypatch)
    torch.manual_seed(11)
    feat32 = torch.randn(N, f)
    if dtype == torch.float32:
        monkeypatch.setenv("VOLTRIX_FP32_MODE", "fp16")
        feat32 = feat32 * 2.0 ** 20
        operand, out_scale, padded, exact = _operand(feat32.cuda())
        assert operand.dtype == torch.float16 and not exact and out_scale is not None and float(out_scale[0]) != 1.0
    else:
        feat32 = feat32.to(dtype).float()           # the caller's data IS fp16 / bfloat16
    feat = feat32.to(dtype).cuda()
    outs = []
    for i in range(4):
        outs.append(_call_with_mode(call, feat, "atomic" if i == 0 else "ticket"))
        assert hybrid.join_error_word() == 0
    assert outs[0].shape == (N, f) and outs[0].dtype == torch.float32
    for out in outs[1:]:
        assert torch.equal(out, outs[0])
    _assert_close(outs[1], indptr, indices, feat32, N, mode)


def test_ticket_steps_on_poisoned_scratch(cuda_device):
    """The second and third call of a handle with every ``torch.empty`` of the step -- C itself, the partial tiles of the cut windows,
    the partial tiles of the cut panel -- filled with 0xFF (NaN): integers, so the product is exact."""
    indptr, indices, two, call = _explicit("ticket_paths_poisoned", "cut_panel")
    gen = torch.Generator(device="cuda").manual_seed(6)
    feat = torch.randint(-3, 4, (N, 128), device="cuda", generator=gen).half()
    want = torch.from_numpy(oracle_np.spmm_csr(indptr, indices, feat.cpu().double().numpy(), N))
    first = _call_with_mode(call, feat, "atomic")
    table = handle_unit_table(two.blk_offsets, two.hspa_packed, N, pairs=True, xcd_ptr=two.window_xcd_ptr)
    assert table.num_slots > 0 and two.plan.parts.num_slots > 0          # both partial-tile buffers exist
    assert torch.equal(first.cpu().double(), want)
    with poisoned(0xFF) as state:
        second = _call_with_mode(call, feat, "ticket")
        third = _call_with_mode(call, feat, "ticket")
        torch.cuda.synchronize()
    assert state.filled > 0
    assert hybrid.join_error_word() == 0
    assert torch.equal(second.cpu().double(), want), "second call: not the exact product of integer operands"
    assert torch.equal(third.cpu().double(), want), "third call: not the exact product of integer operands"


def _features(count, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return [torch.randn(N, 128, device="cuda", generator=gen).half() for _ in range(count)]


def _assert_tickets_clean(tickets, what):
    """After a step: error word and header zero, every block written once by each of at most two producers."""
    words = tickets.cpu()
    blocks = (N + 15) // 16
    assert int(words[0]) == 0, f"{what}: error word {int(words[0])}"
    assert not words[1:hybrid.TICKET_HEADER].any() and not words[hybrid.TICKET_HEADER + blocks:].any(), what
    body = words[hybrid.TICKET_HEADER:hybrid.TICKET_HEADER + blocks]
    assert bool(((body == 2) | (body == 3)).all()), (what, body.tolist())


def test_captured_ticket_step_replays(cuda_device):
    """A captured ticket step is right on its second and third replay only if the zeroing of its ticket buffer is part of the graph."""
    indptr, indices, two, call = _explicit("ticket_paths_graph", "cut_panel")
    feats = _features(4, 21)
    static_in = feats[0].clone()
    _call_with_mode(call, static_in, "atomic")
    _call_with_mode(call, static_in, "ticket")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    hybrid.LAST_JOIN["mode"] = hybrid.LAST_JOIN["tickets"] = None
    with torch.cuda.graph(graph):
        static_out = call(static_in)
    assert hybrid.LAST_JOIN["mode"] == "ticket"
    tickets = hybrid.LAST_JOIN["tickets"]
    for k, feat in enumerate(feats[1:], 1):
        static_in.copy_(feat)
        static_out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        _assert_tickets_clean(tickets, f"replay {k}")
        replayed = static_out.clone()
        eager = _call_with_mode(call, feat, "ticket")
        assert torch.equal(replayed, eager), f"replay {k}"
    _assert_close(replayed, indptr, indices, feats[-1].float().cpu(), N, "fp16")


def test_graphed_spmm_replays_a_ticket_step(cuda_device, monkeypatch):
    """``GraphedSpMM`` warms with two calls and captures the third: a ticket step, replayed for every call."""
    indptr, indices, two, call, handle = _side_car("ticket_paths_graphed", monkeypatch)
    feats = _features(3, 22)
    hybrid.LAST_JOIN["mode"] = hybrid.LAST_JOIN["tickets"] = None
    op = GraphedSpMM(*handle, N, len(indices), feats[0])
    assert hybrid.LAST_JOIN["mode"] == "ticket"
    tickets = hybrid.LAST_JOIN["tickets"]
    for k, feat in enumerate(feats):
        op.static_output.fill_(float("nan"))
        got = op(feat).clone()
        torch.cuda.synchronize()
        _assert_tickets_clean(tickets, f"call {k}")
        assert torch.equal(got, _call_with_mode(call, feat, "ticket")), f"call {k}"
    _assert_close(got, indptr, indices, feats[-1].float().cpu(), N, "fp16")


def test_ticket_steps_on_two_user_streams(cuda_device):
    """One handle, two streams, five ticket steps each, interleaved from the host without a sync in between: every call has a
    ticket buffer of its own (the side stream is shared), so all ten results are the serial ones."""
    indptr, indices, two, call = _explicit("ticket_paths_streams")
    feats = [_features(5, 31), _features(5, 32)]
    _call_with_mode(call, feats[0][0], "atomic")
    serial = [[_call_with_mode(call, feat, "ticket") for feat in per_stream] for per_stream in feats]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs, tickets = [[], []], [[], []]
    for i in range(5):
        for k, stream in enumerate(streams):
            with torch.cuda.stream(stream):
                outs[k].append(_call_with_mode(call, feats[k][i], "ticket"))
                tickets[k].append(hybrid.LAST_JOIN["tickets"])
    torch.cuda.synchronize()
    for k in range(2):
        for i in range(5):
            assert torch.equal(outs[k][i], serial[k][i]), (k, i)
            _assert_tickets_clean(tickets[k][i], f"stream {k} call {i}")
    assert len({t.data_ptr() for per_stream in tickets for t in per_stream}) == 10
    _assert_close(outs[1][4], indptr, indices, feats[1][4].float().cpu(), N, "fp16")


def test_autograd_forward_and_backward_twice(cuda_device, monkeypatch):
    """``voltrix.autograd.SpMM`` builds both of its handles with ``csr_preprocess_device``: with the side-car forced, A and A^T are
    both two-level handles (256-row panels: the panel side dominates both at the default tau), so each product takes the atomic join
    in the first pass and the ticket join in the second.  fp32 features and gradients: both products run on the scaled fp16 operand."""
    monkeypatch.setenv("VOLTRIX_HYBRID", "1")
    monkeypatch.setenv("VOLTRIX_HYBRID_MIN_SHARE", "0")
    monkeypatch.setenv("VOLTRIX_FP32_MODE", "fp16")
    indptr, indices = _graph(True, N)
    op = voltrix.autograd.SpMM(torch.from_numpy(indptr), torch.from_numpy(indices), N, hash_tag="ticket_paths_autograd")
    two_level = [voltrix.two_level_of(h[1]) for h in (op.handle, op.handle_t)]
    assert all(t is not None and t.plan.num_ksteps > 0 and t.plan.num_resid_edges > 0 for t in two_level)
    torch.manual_seed(41)
    x32, g32 = torch.randn(N, 128), torch.randn(N, 128)
    x, g = x32.cuda().requires_grad_(), g32.cuda()
    modes, grads, outs = [], [], []
    for _ in range(2):
        hybrid.LAST_JOIN["mode"] = None
        y = op(x)
        modes.append(hybrid.LAST_JOIN["mode"])
        hybrid.LAST_JOIN["mode"] = None
        y.backward(g)
        modes.append(hybrid.LAST_JOIN["mode"])
        assert hybrid.join_error_word() == 0
        outs.append(y.detach())
        grads.append(x.grad.clone())
        x.grad = None
    assert modes == ["atomic", "atomic", "ticket", "ticket"], modes        # forward, backward; forward, backward
    assert torch.equal(outs[0], outs[1]) and torch.equal(grads[0], grads[1])
    _assert_close(outs[1], indptr, indices, x32, N, "fp16-scaled")
    at = sp.csr_matrix((np.ones(len(indices), np.float32), indices, indptr), shape=(N, N)).T.tocsr()
    at.sort_indices()
    _assert_close(grads[1], at.indptr.astype(np.int32), at.indices.astype(np.int32), g32, N, "fp16-scaled")
