"""Child process of tests/test_spmm_rel_host.py: the host-side argument contract of ``voltrix_spmm_rel_csr``,
``voltrix_spmm_rel_contract_csr`` and ``voltrix_spmm_rel_dots_csr`` on 16-byte-aligned HOST buffers, in a process that cannot see a
device -- a call that slips past a missing check ends at the runtime's "no device" (2), not in a kernel launch on host pointers.  The
protocol of tests/spmm_edge_abi_worker.py: the parent hides the devices (HIP_VISIBLE_DEVICES=-1); this process asks the HIP runtime
for its device count before the first library call and makes none unless that count is zero (exit code 3).

    python spmm_rel_abi_worker.py

Prints ``{"devices": n}`` first, then one JSON line ``{"id": ..., "rc": ...}`` per case as it returns, then ``{"done": count}``.
``cases()`` -- ``[(id, symbol, {parameter: value}, expected code)]`` -- needs no library: the parent imports it for the expectations.
The three entry points RETURN their code.  No torch, no package import: voltrix/capi.py is loaded by path.
"""
import ctypes
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
EXIT_DEVICE_VISIBLE = 3
OK, BAD, LAUNCH = 0, 1, 2          # VOLTRIX_OK, VOLTRIX_ERR_BAD_SHAPE, VOLTRIX_ERR_LAUNCH (here: no device)
SET, NULL = "set", None            # a pointer parameter: its aligned buffer, NULL, or ("off", bytes) past the buffer's start
FP32, FP16, BF16 = 0, 1, 2
MAX_TYPES, MAX_BASES = 65536, 1024

FORWARD = "voltrix_spmm_rel_csr"
CONTRACT = "voltrix_spmm_rel_contract_csr"
DOTS = "voltrix_spmm_rel_dots_csr"
SYMBOLS = (FORWARD, CONTRACT, DOTS)
# parameter order of the header; the baseline of each symbol is a valid call (answered with "no device")
PARAMS = {
    FORWARD: [("indptr", SET), ("indices", SET), ("etype", SET), ("weight", SET), ("num_rows", 4), ("num_entries", 8),
              ("embedding_dim", 8), ("num_types", 3), ("num_bases", 2), ("input", SET), ("dtype", FP32), ("coef", SET), ("output", SET),
              ("stream", NULL)],
    CONTRACT: [("t_indptr", SET), ("t_indices", SET), ("order", SET), ("etype", SET), ("weight", SET), ("num_cols", 4),
               ("num_entries", 8), ("embedding_dim", 8), ("num_types", 3), ("num_bases", 2), ("grad_out", SET), ("coef", SET),
               ("output", SET), ("stream", NULL)],
    DOTS: [("indptr", SET), ("indices", SET), ("weight", SET), ("num_rows", 4), ("num_entries", 8), ("embedding_dim", 8),
           ("num_bases", 2), ("grad_out", SET), ("feat", SET), ("dtype", FP32), ("output", SET), ("stream", NULL)],
}
ROWS = {FORWARD: "num_rows", CONTRACT: "num_cols", DOTS: "num_rows"}
REQUIRED4 = {FORWARD: ("indptr", "indices", "etype"), CONTRACT: ("t_indptr", "t_indices", "etype"), DOTS: ("indptr", "indices")}
NULLABLE4 = {FORWARD: ("weight",), CONTRACT: ("order", "weight"), DOTS: ("weight",)}          # 4-byte loads, may be NULL
SIXTEEN = {FORWARD: ("input", "coef", "output"), CONTRACT: ("grad_out", "coef", "output"), DOTS: ("grad_out", "feat", "output")}
POINTERS = {s: REQUIRED4[s] + NULLABLE4[s] + SIXTEEN[s] for s in SYMBOLS}


def cases():
    out = []

    def add(symbol, what, expected, **overrides):
        out.append((f"{symbol}::{what}", symbol, overrides, expected))

    for symbol in SYMBOLS:
        add(symbol, "baseline", LAUNCH)
        for p in REQUIRED4[symbol] + SIXTEEN[symbol]:
            add(symbol, f"{p}=NULL", BAD, **{p: NULL})
        for p in NULLABLE4[symbol]:
            add(symbol, f"{p}=NULL", LAUNCH, **{p: NULL})
        add(symbol, "every nullable pointer NULL", LAUNCH, **{p: NULL for p in NULLABLE4[symbol]})
        for p in REQUIRED4[symbol] + NULLABLE4[symbol]:
            add(symbol, f"{p}+2", BAD, **{p: ("off", 2)})
        for p in SIXTEEN[symbol]:
            for off in (4, 8):
                add(symbol, f"{p}+{off}", BAD, **{p: ("off", off)})
        add(symbol, "rows=-1", BAD, **{ROWS[symbol]: -1})
        add(symbol, "embedding_dim=-1", BAD, embedding_dim=-1)
        add(symbol, "embedding_dim=V+1 fp32", BAD, embedding_dim=5)
        add(symbol, "num_entries=-1", BAD, num_entries=-1)
        add(symbol, "num_entries=2^31", BAD, num_entries=2 ** 31)
        add(symbol, "num_entries=2^31-1", LAUNCH, num_entries=2 ** 31 - 1)
        add(symbol, "num_bases=-1", BAD, num_bases=-1)
        add(symbol, "num_bases=limit", LAUNCH, num_bases=MAX_BASES)
        add(symbol, "num_bases=limit+1", BAD, num_bases=MAX_BASES + 1)
        # nothing to do: no launch, and no pointer is looked at
        add(symbol, "rows=0", OK, **{ROWS[symbol]: 0})
        add(symbol, "embedding_dim=0", OK, embedding_dim=0)
        add(symbol, "num_bases=0", OK, num_bases=0)
        add(symbol, "rows=0 every pointer NULL", OK, **{ROWS[symbol]: 0}, **{p: NULL for p in POINTERS[symbol]})
        add(symbol, "num_bases=0 but num_entries=2^31", BAD, num_bases=0, num_entries=2 ** 31)
    for symbol in (FORWARD, CONTRACT):
        add(symbol, "num_types=0", BAD, num_types=0)
        add(symbol, "num_types=limit", LAUNCH, num_types=MAX_TYPES)
        add(symbol, "num_types=limit+1", BAD, num_types=MAX_TYPES + 1)
        add(symbol, "both limits", LAUNCH, num_types=MAX_TYPES, num_bases=MAX_BASES)
    for symbol in (FORWARD, DOTS):
        for d in (-1, 3):
            add(symbol, f"dtype={d}", BAD, dtype=d)
        for d in (FP16, BF16):
            add(symbol, f"dtype={d}", LAUNCH, dtype=d)
            add(symbol, f"dtype={d} embedding_dim=V+1", BAD, dtype=d, embedding_dim=9)
            add(symbol, f"dtype={d} embedding_dim=4", BAD, dtype=d, embedding_dim=4)
    add(FORWARD, "num_entries=0", LAUNCH, num_entries=0)            # the rows are zero-filled by the kernel
    add(CONTRACT, "num_entries=0", LAUNCH, num_entries=0)
    add(CONTRACT, "embedding_dim=4", LAUNCH, embedding_dim=4)       # grad_out is fp32: pieces of 4
    add(DOTS, "num_entries=0", OK, num_entries=0)                   # no entry, no dot
    assert len({c[0] for c in out}) == len(out)
    return out


def say(record):
    sys.stdout.write(json.dumps(record) + "\n")
    sys.stdout.flush()


def visible_devices(lib) -> int:
    """hipGetDeviceCount of the runtime the library itself is linked against (resolved through the library's handle)."""
    fn = lib.hipGetDeviceCount
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.POINTER(ctypes.c_int)]
    count = ctypes.c_int(0)
    status = fn(ctypes.byref(count))          # hipErrorNoDevice leaves the count at 0
    return count.value if status == 0 else 0


def call(lib, symbol, overrides):
    assert not set(overrides) - {p for p, _ in PARAMS[symbol]}, overrides
    keep, args = [], []
    for name, value in PARAMS[symbol]:
        value = overrides.get(name, value)
        if name in POINTERS[symbol]:
            if value is not NULL:
                buf = ctypes.create_string_buffer(4096 + 16)
                keep.append(buf)
                base = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
                value = ctypes.c_void_p(base if value == SET else base + value[1])
        args.append(value)
    return int(getattr(lib, symbol)(*args))


def main() -> int:
    spec = importlib.util.spec_from_file_location("voltrix_capi_by_path", os.path.join(REPO, "voltrix-spmm_amd", "voltrix", "capi.py"))
    capi = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(capi)
    lib = capi.lib()
    devices = visible_devices(lib)
    say({"devices": devices})
    if devices != 0:
        say({"refused": f"{devices} device(s) visible: no library call is made"})
        return EXIT_DEVICE_VISIBLE
    count = 0
    for case_id, symbol, overrides, _ in cases():
        say({"id": case_id, "rc": call(lib, symbol, overrides)})
        count += 1
    say({"done": count})
    return 0


if __name__ == "__main__":
    sys.exit(main())
