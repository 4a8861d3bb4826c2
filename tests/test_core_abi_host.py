"""CPU: the host-side argument contract of EVERY entry point of the C ABI that launches -- the block-format, stream, panel and fused
launchers with their combine passes, the CSR row-gather kernel, the table and plan builders and the helpers, and the operators on a
device CSR: attention, max / min / mean, sampling (tests/core_abi_cases.py has a row per entry point).  Every bad argument is answered
on the host, before any launch: a null or misaligned pointer, a size below zero or beyond its limit, an enum outside its range, a
float that is not finite and a width off the grid with VOLTRIX_ERR_BAD_SHAPE (VOLTRIX_ERR_OVERFLOW / _BAD_CONFIG where the header
says so), "nothing to do" with VOLTRIX_OK.

The calls are made by ONE child process that cannot see a device (tests/core_abi_worker.py; HIP_VISIBLE_DEVICES=-1 on top of this
process's own environment): where a check is missing the call ends at the runtime's "no device" (VOLTRIX_ERR_LAUNCH) instead of in a
kernel on host pointers -- on a machine with a GPU as well.  A child that still sees a device makes no call and the tests FAIL."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

from conftest import REPO

import core_abi_cases as table
from voltrix import capi

WORKER = os.path.join(REPO, "tests", "core_abi_worker.py")
NAMES = {0: "VOLTRIX_OK", 1: "VOLTRIX_ERR_BAD_SHAPE", 2: "VOLTRIX_ERR_LAUNCH", 3: "VOLTRIX_ERR_BAD_CONFIG", 4: "VOLTRIX_ERR_OVERFLOW",
         5: "VOLTRIX_ERR_DUPLICATE"}


@pytest.fixture(scope="module")
def answers():
    """``{case id: return code}`` of every case, from one child."""
    run = subprocess.run([sys.executable, WORKER], env={**os.environ, "HIP_VISIBLE_DEVICES": "-1"}, capture_output=True, text=True,
                         timeout=600)
    lines = [json.loads(line) for line in run.stdout.splitlines() if line.startswith("{")]
    assert lines and "devices" in lines[0], f"the child said nothing (exit code {run.returncode}):\n{run.stderr[-3000:]}"
    assert lines[0]["devices"] == 0 and run.returncode != 3, \
        f"the child sees {lines[0]['devices']} device(s) with HIP_VISIBLE_DEVICES=-1: it made no library call"
    got = {line["id"]: line["rc"] for line in lines if "id" in line}
    if run.returncode != 0 or "done" not in lines[-1]:
        order = [c["id"] for c in table.cases()]
        pytest.fail(f"the child ended with exit code {run.returncode} in the call after {len(got)} answers -- "
                    f"{order[len(got)] if len(got) < len(order) else 'a size function'}:\n{run.stderr[-3000:]}")
    assert lines[-1]["done"] == len(got) == len(table.cases()) + len(table.SIZE_FUNCTIONS)
    return got


def test_every_launch_symbol_has_a_contract_test():
    """In-process, no library call: the table's rows are the symbols of the binding that return nothing and end in a stream and the
    return-code slot (or, for the reference's host preprocess, a pointer and the slot) -- by their shape, not by their name.  Today
    that is every ``voltrix_launch_*`` and the weighted sampler; a symbol that breaks the rule fails here instead of being left out."""
    launching = {name for name, (restype, argtypes) in capi.SIGNATURES.items()
                 if restype is None and argtypes[-2:] == [ctypes.c_void_p, capi._RC_P]}
    rows = set(table.ROWS)
    assert not launching - rows, f"entry points without a row in tests/core_abi_cases.py: {sorted(launching - rows)}"
    assert not rows - launching, f"rows that are no launching symbol of capi.SIGNATURES: {sorted(rows - launching)}"
    assert launching == {name for name in capi.SYMBOLS if name.startswith("voltrix_launch_")} | {"voltrix_sample_neighbors_weighted"}


def test_every_launcher_with_nnz_refuses_two_to_the_31_on_the_host(answers):
    """Every launcher the header declares with an ``int64_t nnz`` has a row whose ``nnz`` is limited to INT_MAX, and no other row has:
    a new launcher that takes nnz belongs there.  The derived call with nnz = 2^31 is refused on the host, before any HIP call."""
    from capi_header import prototypes

    with_nnz = {name for name, (returns, params) in prototypes().items() if returns is None and (ctypes.c_int64, "nnz") in params}
    limited = {name for name, r in table.ROWS.items()
               if any(p == "nnz" and isinstance(role, table.N) and role.hi == table.INT_MAX for p, role in r["params"])}
    assert with_nnz == limited and len(limited) == 17, sorted(with_nnz ^ limited)
    for name in sorted(limited):
        assert answers[f"{name}::nnz={2 ** 31}"] == table.BAD, name


def test_rows_follow_the_binding():
    """A row has one role per parameter of ``capi.SIGNATURES``: pointer roles on ``void*`` (or the typed host pointer), the return-code
    slot last, values elsewhere; and the baseline of a required pointer is set, of an optional one NULL."""
    for name, r in table.ROWS.items():
        restype, argtypes = capi.SIGNATURES[name]
        assert restype is None and len(argtypes) == len(r["params"]), name
        assert r["params"][-1][1] is table.RC and argtypes[-1] is capi._RC_P, name
        assert len({p for p, _ in r["params"]}) == len(r["params"]), name
        for (pname, role), ctype in zip(r["params"][:-1], argtypes[:-1]):
            pointer = ctype in (ctypes.c_void_p, capi._RC_P)
            assert pointer == (role.kind in ("pointer", "stream")), (name, pname)
            if role.kind == "value":      # the value arrives as the binding's type: a float as a float, an integer inside its range
                assert isinstance(role.value, float) == (ctype in (ctypes.c_float, ctypes.c_double)), (name, pname)
                assert isinstance(role.value, float) or ctype(role.value).value == role.value, (name, pname)
            if role.kind == "pointer":
                assert role.value == (table.NULL if isinstance(role, table.O) else table.SET), (name, pname)
                assert role.align in (None, 4, 8, 16), (name, pname)
        assert r["baseline"] not in (1, 3, 4, 5), name
        assert any(isinstance(role, table.P) and not isinstance(role, (table.O, table.E)) for _, role in r["params"]), name


def test_the_baseline_of_every_row_is_not_refused(answers):
    """Otherwise a bad call could "pass" because the call was refused for another reason.  Without a device a valid call that would
    launch answers VOLTRIX_ERR_LAUNCH; the rows that answer something else say why."""
    for name, r in table.ROWS.items():
        rc = answers[f"{name}::baseline"]
        assert rc not in (1, 3, 4, 5) and rc == r["baseline"], f"{name}: baseline answered {rc} ({NAMES.get(rc)}), the row says {r['baseline']}"


def test_every_derived_call_is_answered_as_the_contract_says(answers):
    wrong = [f"{c['id']}: {answers[c['id']]} ({NAMES.get(answers[c['id']], '?')}) where {c['expect']} ({NAMES[c['expect']]}) is expected"
             for c in table.cases() if answers[c["id"]] != c["expect"]]
    assert not wrong, f"{len(wrong)} of {len(table.cases())} calls:\n" + "\n".join(wrong)


def test_the_table_derives_the_cases_the_contract_names():
    """The derivation itself: per kind of role the calls that have to be there, on one row that has them all."""
    ids = {c["id"]: c for c in table.cases()}
    name = "voltrix_launch_spmm_f16_sched"
    for what, expect in (("blk_offsets=NULL", 1), ("input=NULL", 1), ("input+4", 1), ("input+8", 1), ("output=NULL", 1),
                         ("hspa_packed=NULL(may be empty)", 2), ("hspa_packed+4", 1), ("hind=NULL(may be empty)", 2),
                         ("num_nodes=-1", 1), ("embedding_dim=-1", 1), ("atomic_out=-1", 1), ("atomic_out=3", 1),
                         ("window_order=set", 2), ("units=set", 2), ("units+4", 1), ("units+8", 1), ("row_map=set", 2),
                         ("width", 1), ("tile_not_instantiated", 3), ("units_without_unit_ptr", 1), ("ticket_join_without_tickets", 1)):
        assert ids[f"{name}::{what}"]["expect"] == expect, what
    assert ids["voltrix_launch_spmm_csr_rows::indptr+2"]["expect"] == 1                      # 4 bytes wanted, off by 2
    assert ids["voltrix_launch_cast_f32_f16_scaled::scale+4"]["expect"] == 1                 # 8 bytes wanted, off by 4
    assert ids[f"voltrix_launch_csr_fill::num_edges={2 ** 31 - 2}"]["expect"] == 4           # num_edges + windows beyond int32
    assert ids[f"voltrix_launch_panel_plan_count::num_cols={2 ** 22 + 1}"]["expect"] == 3    # the two-level format is not built for it
    assert ids["voltrix_launch_chol_inv_transposed::k=0"]["expect"] == 1 and ids["voltrix_launch_chol_inv_transposed::k=65"]["expect"] == 1
    assert ids[f"voltrix_launch_sddmm_csr::nnz={2 ** 31 - 1}(the limit)"]["expect"] == 2      # an entry count limited to INT_MAX ...
    assert ids[f"voltrix_launch_sddmm_csr::nnz={2 ** 31}"]["expect"] == 1                     # ... and the first value beyond it
    assert ids["voltrix_sample_neighbors_weighted::cum+4"]["expect"] == 1                    # int64 weights: 8 bytes wanted
    for what in ("scale=inf", "scale=-inf", "scale=nan", "keep_scale=-1.0", f"keep_scale={-2.0 ** -140!r}"):   # floats, named by repr
        assert ids[f"voltrix_launch_attn_aggregate_dropout_csr::{what}"]["expect"] == 1, what
    assert ids["voltrix_launch_subgraph_count::group=12"]["expect"] == 1 and ids["voltrix_launch_subgraph_count::group=16"]["expect"] == 2
    # the 1,163 cases of the table before it held every entry point, and the 1,069 distinct calls the per-operator host tests made
    assert len(ids) >= 1163 + 1069


def test_size_functions(answers):
    """A negative argument gives the documented answer; a workspace the header calls 16-byte aligned has a size that is a multiple
    of 16, at zero as well; the workspaces the table calls required are never empty."""
    for name, args, expect in table.SIZE_FUNCTIONS:
        got = answers[f"{name}{args}"]
        if expect == table.ALIGNED:
            assert got >= 0 and got % 16 == 0, (name, args, got)
        elif expect == table.POSITIVE_ALIGNED:
            assert got > 0 and got % 16 == 0, (name, args, got)
        else:
            assert got == expect, (name, args, got)


# ---- the combinations the launch functions refuse that no entry point of the C ABI can express (the ticket forms take no row_map, the
# ---- fp32 and weighted tiles have no ticket entry point, the slab window is an argument of the launch functions alone): a header-only
# ---- host program, compiled here, run as a child that cannot see a device and asks for the device count first, like the worker
COMBINATIONS = r"""
#include <cstdio>
#include "voltrix/spmm_kernels.hpp"
using namespace voltrix;
alignas(16) static char buf[8][4096];
int main() {
  int devices = 0;
  if (hipGetDeviceCount(&devices) != hipSuccess) devices = 0;
  printf("devices %d\n", devices);
  if (devices != 0) return 3;
  const int* blk = (const int*)buf[0]; const uint32_t* packed = (const uint32_t*)buf[1]; const int* hind = (const int*)buf[2];
  const void* in = buf[3]; float* out = (float*)buf[4]; int* tickets = (int*)buf[5]; const int* row_map = (const int*)buf[6];
  const int* cuts = (const int*)buf[0]; const float* partials = (const float*)buf[1];
  using F16 = SpmmTile<64, 3, 4, 2, false>;
  using F32 = SpmmTile<64, 3, 1, 4, false>;
  using W16 = SpmmTile<64, 3, 4, 2, false, true>;
#define SPMM(T, F, ATOMIC, ROW_MAP, VALUES, FIRST, COUNT, TICKETS)                                                              \
  launch_spmm_tc16<T>(blk, packed, hind, 32, F, in, out, nullptr, nullptr, nullptr, ATOMIC, nullptr, nullptr, 0, nullptr, ROW_MAP, \
                      VALUES, 1, FIRST, COUNT, 0, kSlabAuto, TICKETS)
  printf("ticket_join %d\n", SPMM(F16, 64, 2, nullptr, nullptr, 0, 0, tickets));
  printf("ticket_join_on_an_fp32_tile %d\n", SPMM(F32, 64, 2, nullptr, nullptr, 0, 0, tickets));
  printf("ticket_join_on_a_weighted_tile %d\n", SPMM(W16, 64, 2, nullptr, buf[7], 0, 0, tickets));
  printf("ticket_join_with_a_row_map %d\n", SPMM(F16, 64, 2, row_map, nullptr, 0, 0, tickets));
  printf("ticket_join_wider_than_the_slab %d\n", SPMM(F16, 128, 2, nullptr, nullptr, 0, 0, tickets));
  printf("weighted_tile_without_values %d\n", SPMM(W16, 64, 0, nullptr, nullptr, 0, 0, nullptr));
  printf("last_slab %d\n", SPMM(F16, 128, 0, nullptr, nullptr, 1, 1, nullptr));
  printf("slabs_past_the_last %d\n", SPMM(F16, 128, 0, nullptr, nullptr, 1, 2, nullptr));
  printf("slab_first_negative %d\n", SPMM(F16, 128, 0, nullptr, nullptr, -1, 1, nullptr));
  printf("slab_count_negative %d\n", SPMM(F16, 128, 0, nullptr, nullptr, 0, -1, nullptr));
  printf("combine_with_tickets %d\n", combine_partials(cuts, 2, partials, out, 32, 64, 1, nullptr, nullptr, tickets));
  printf("combine_with_tickets_and_a_row_map %d\n", combine_partials(cuts, 2, partials, out, 32, 64, 1, nullptr, row_map, tickets));
  // the launch function itself takes a NULL operand (an operator without columns: its callers state the rows); the C ABI's
  // block-format entry points, which cannot state them, refuse it (the table)
  printf("null_operand_at_the_launch_function %d\n",
         launch_spmm_tc16<F16>(blk, packed, hind, 32, 64, nullptr, out, nullptr));
  return 0;
}
"""
COMBINATIONS_EXPECTED = {
    "ticket_join": 2, "ticket_join_on_an_fp32_tile": 1, "ticket_join_on_a_weighted_tile": 1, "ticket_join_with_a_row_map": 1,
    "ticket_join_wider_than_the_slab": 1, "weighted_tile_without_values": 1, "last_slab": 2, "slabs_past_the_last": 1,
    "slab_first_negative": 1, "slab_count_negative": 1, "combine_with_tickets": 2, "combine_with_tickets_and_a_row_map": 1,
    "null_operand_at_the_launch_function": 2,
}


def test_combinations_only_the_launch_functions_can_express(tmp_path):
    src = tmp_path / "combinations.hip"
    src.write_text(COMBINATIONS)
    inc = os.path.join(REPO, "voltrix-spmm_amd", "voltrix", "include")
    build = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17", "-I", inc, str(src), "-o",
                            str(tmp_path / "combinations")], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(tmp_path / "combinations")], env={**os.environ, "HIP_VISIBLE_DEVICES": "-1"}, capture_output=True,
                         text=True, timeout=120)
    lines = dict(line.rsplit(" ", 1) for line in run.stdout.splitlines())
    assert lines.get("devices") == "0" and run.returncode == 0, f"exit code {run.returncode}:\n{run.stdout}\n{run.stderr[-2000:]}"
    del lines["devices"]
    assert {k: int(v) for k, v in lines.items()} == COMBINATIONS_EXPECTED
