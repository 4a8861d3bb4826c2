"""Child process of tests/test_spmm_fp8_host.py: the host-side argument contract of ``voltrix_quantize_fp8_rows`` and
``voltrix_spmm_fp8_csr`` on 16-byte-aligned HOST buffers, in a process that cannot see a device -- a call that slips past a missing
check ends at the runtime's "no device" (2), not in a kernel launch on host pointers.  The protocol of tests/spmm_edge_abi_worker.py:
the parent hides the devices (HIP_VISIBLE_DEVICES=-1); this process asks the HIP runtime for its device count before the first library
call and makes none unless that count is zero (exit code 3).

    python spmm_fp8_abi_worker.py

Prints ``{"devices": n}`` first, then one JSON line ``{"id": ..., "rc": ...}`` per case as it returns, then ``{"done": count}``.
``cases()`` -- ``[(id, symbol, {parameter: value}, expected code)]`` -- needs no library: the parent imports it for the expectations.
The two entry points RETURN their code.  No torch, no package import: voltrix/capi.py is loaded by path.
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

QUANTIZE = "voltrix_quantize_fp8_rows"
SPMM = "voltrix_spmm_fp8_csr"
SYMBOLS = (QUANTIZE, SPMM)
# parameter order of the header; the baseline of each symbol is a valid call (answered with "no device")
PARAMS = {
    QUANTIZE: [("input", SET), ("dtype", FP32), ("num_rows", 4), ("embedding_dim", 20), ("input_ld", 20), ("inv_scale", SET),
               ("output", SET), ("output_ld", 32), ("stream", NULL)],
    SPMM: [("indptr", SET), ("indices", SET), ("values", SET), ("num_rows", 4), ("embedding_dim16", 32), ("input", SET),
           ("scale", SET), ("output", SET), ("out_dtype", FP32), ("xcd_ranges", 1), ("num_entries", 8), ("stream", NULL)],
}
ROWS = "num_rows"
WIDTH = {QUANTIZE: "embedding_dim", SPMM: "embedding_dim16"}
REQUIRED4 = {QUANTIZE: (), SPMM: ("indptr", "indices")}                 # 4-byte loads
NULLABLE4 = {QUANTIZE: (), SPMM: ("values",)}                           # 4-byte loads, may be NULL
SIXTEEN = {QUANTIZE: ("input", "inv_scale", "output"), SPMM: ("input", "scale", "output")}
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
        for p in REQUIRED4[symbol] + NULLABLE4[symbol]:
            add(symbol, f"{p}+2", BAD, **{p: ("off", 2)})
        for p in SIXTEEN[symbol]:
            for off in (4, 8):
                add(symbol, f"{p}+{off}", BAD, **{p: ("off", off)})
        add(symbol, "rows=-1", BAD, **{ROWS: -1})
        add(symbol, "width=-1", BAD, **{WIDTH[symbol]: -1})
        # nothing to do: no launch, and no pointer is looked at
        add(symbol, "rows=0", OK, **{ROWS: 0})
        add(symbol, "rows=0 every pointer NULL", OK, **{ROWS: 0}, **{p: NULL for p in POINTERS[symbol]})
    # the quantiser: the input's type, the two row strides
    add(QUANTIZE, "embedding_dim=0", OK, embedding_dim=0, input_ld=0)
    add(QUANTIZE, "embedding_dim=0 every pointer NULL", OK, embedding_dim=0, **{p: NULL for p in POINTERS[QUANTIZE]})
    for d in (-1, 3):
        add(QUANTIZE, f"dtype={d}", BAD, dtype=d)
    for d in (FP16, BF16):
        add(QUANTIZE, f"dtype={d}", LAUNCH, dtype=d)
    add(QUANTIZE, "dtype=-1 rows=0", BAD, dtype=-1, num_rows=0)          # sizes and types come before "nothing to do"
    add(QUANTIZE, "input_ld<embedding_dim", BAD, input_ld=19)
    add(QUANTIZE, "input_ld=-1", BAD, input_ld=-1)
    add(QUANTIZE, "input_ld wider", LAUNCH, input_ld=48)
    add(QUANTIZE, "output_ld<F16", BAD, output_ld=16)
    add(QUANTIZE, "output_ld=F16+8", BAD, output_ld=40)
    add(QUANTIZE, "output_ld wider", LAUNCH, output_ld=64)
    add(QUANTIZE, "embedding_dim=1", LAUNCH, embedding_dim=1, input_ld=1, output_ld=16)
    add(QUANTIZE, "embedding_dim=16", LAUNCH, embedding_dim=16, input_ld=16, output_ld=16)
    # the aggregation: the width in whole pieces, the entry count, the output's type
    add(SPMM, "embedding_dim16=0", OK, embedding_dim16=0)
    add(SPMM, "embedding_dim16=0 every pointer NULL", OK, embedding_dim16=0, **{p: NULL for p in POINTERS[SPMM]})
    for width in (17, 8, 24):
        add(SPMM, f"embedding_dim16={width}", BAD, embedding_dim16=width)
    add(SPMM, "embedding_dim16=17 rows=0", BAD, embedding_dim16=17, num_rows=0)
    add(SPMM, "embedding_dim16=16", LAUNCH, embedding_dim16=16)
    add(SPMM, "embedding_dim16=1040", LAUNCH, embedding_dim16=1040)
    add(SPMM, "num_entries=-1", BAD, num_entries=-1)
    add(SPMM, "num_entries=2^31", BAD, num_entries=2 ** 31)
    add(SPMM, "num_entries=2^31-1", LAUNCH, num_entries=2 ** 31 - 1)
    add(SPMM, "num_entries=0", LAUNCH, num_entries=0)                   # every row is written as 0 by the kernel
    add(SPMM, "num_entries=-1 rows=0", BAD, num_entries=-1, num_rows=0)
    for d in (-1, 3):
        add(SPMM, f"out_dtype={d}", BAD, out_dtype=d)
    for d in (FP16, BF16):
        add(SPMM, f"out_dtype={d}", LAUNCH, out_dtype=d)
    add(SPMM, "xcd_ranges=0", LAUNCH, xcd_ranges=0)
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
