"""Child process of tests/test_spmm_edge_host.py: the host-side argument contract of ``voltrix_spmm_edge_csr`` and
``voltrix_spmm_edge_grad_efeat_csr`` on 16-byte-aligned HOST buffers, in a process that cannot see a device -- a call that slips past
a missing check ends at the runtime's "no device" (2), not in a kernel launch on host pointers.  The protocol of
tests/core_abi_worker.py: the parent hides the devices (HIP_VISIBLE_DEVICES=-1); this process asks the HIP runtime for its device count
before the first library call and makes none unless that count is zero (exit code 3).

    python spmm_edge_abi_worker.py

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
MUL, ADD, ADD_RELU, COPY, GATE = 0, 1, 2, 3, 4

FORWARD = "voltrix_spmm_edge_csr"
GRAD = "voltrix_spmm_edge_grad_efeat_csr"
# parameter order of the header; the baseline of each symbol is a valid call (answered with "no device")
PARAMS = {
    FORWARD: [("indptr", SET), ("indices", SET), ("order", SET), ("num_rows", 4), ("num_entries", 8), ("embedding_dim", 8),
              ("input", SET), ("input_dtype", FP32), ("efeat", SET), ("efeat_dtype", FP32), ("self", SET), ("op", MUL),
              ("output", SET), ("stream", NULL)],
    GRAD: [("indptr", SET), ("indices", SET), ("num_rows", 4), ("num_entries", 8), ("embedding_dim", 8), ("grad_out", SET),
           ("feat", SET), ("efeat", SET), ("dtype", FP32), ("op", ADD_RELU), ("output", SET), ("stream", NULL)],
}
POINTERS = {FORWARD: ("indptr", "indices", "order", "input", "efeat", "self", "output"),
            GRAD: ("indptr", "indices", "grad_out", "feat", "efeat", "output")}
INDEX_ARRAYS = {FORWARD: ("indptr", "indices", "order"), GRAD: ("indptr", "indices")}          # 4-byte loads
SIXTEEN = {FORWARD: ("input", "efeat", "self", "output"), GRAD: ("grad_out", "feat", "efeat", "output")}


def cases():
    out = []

    def add(symbol, what, expected, **overrides):
        out.append((f"{symbol}::{what}", symbol, overrides, expected))

    for symbol in (FORWARD, GRAD):
        add(symbol, "baseline", LAUNCH)
        for p in INDEX_ARRAYS[symbol]:
            add(symbol, f"{p}+2", BAD, **{p: ("off", 2)})
        for p in SIXTEEN[symbol]:
            for off in (4, 8):
                add(symbol, f"{p}+{off}", BAD, **{p: ("off", off)})
        add(symbol, "num_rows=-1", BAD, num_rows=-1)
        add(symbol, "embedding_dim=-1", BAD, embedding_dim=-1)
        add(symbol, "embedding_dim=V+1 fp32", BAD, embedding_dim=5)
        add(symbol, "num_entries=-1", BAD, num_entries=-1)
        add(symbol, "num_entries=2^31", BAD, num_entries=2 ** 31)
        add(symbol, "num_entries=2^31-1", LAUNCH, num_entries=2 ** 31 - 1)
        add(symbol, "op=-1", BAD, op=-1)
        add(symbol, "num_rows=0", OK, num_rows=0)
        add(symbol, "embedding_dim=0", OK, embedding_dim=0)
    # ---- the forward: required pointers, ops, dtype pairs
    for p in ("indptr", "indices", "efeat", "output"):
        add(FORWARD, f"{p}=NULL", BAD, **{p: NULL})
    add(FORWARD, "op=5", BAD, op=GATE + 1)
    for op in (ADD, ADD_RELU, COPY, GATE):
        add(FORWARD, f"op={op}", LAUNCH, op=op)
    for op in (MUL, ADD, ADD_RELU, GATE):
        add(FORWARD, f"op={op} input=NULL", BAD, op=op, input=NULL)
    add(FORWARD, "copy input=NULL", LAUNCH, op=COPY, input=NULL)
    add(FORWARD, "copy input=NULL self=NULL order=NULL", LAUNCH, op=COPY, input=NULL, self=NULL, order=NULL)
    add(FORWARD, "gate self=NULL", BAD, op=GATE, self=NULL)
    add(FORWARD, "mul self=NULL", LAUNCH, self=NULL)
    add(FORWARD, "order=NULL", LAUNCH, order=NULL)
    for d in (-1, 3):
        add(FORWARD, f"input_dtype={d}", BAD, input_dtype=d)
        add(FORWARD, f"efeat_dtype={d}", BAD, efeat_dtype=d)
        add(FORWARD, f"copy efeat_dtype={d}", BAD, op=COPY, efeat_dtype=d)
    for pair in ((FP32, FP16), (FP32, BF16), (FP16, FP16), (BF16, BF16)):
        add(FORWARD, f"pair={pair}", LAUNCH, input_dtype=pair[0], efeat_dtype=pair[1])
        add(FORWARD, f"pair={pair} embedding_dim=V+1", BAD, input_dtype=pair[0], efeat_dtype=pair[1], embedding_dim=9)
        add(FORWARD, f"pair={pair} embedding_dim=4", BAD, input_dtype=pair[0], efeat_dtype=pair[1], embedding_dim=4)
    for pair in ((FP16, FP32), (BF16, FP32), (FP16, BF16), (BF16, FP16)):
        add(FORWARD, f"pair={pair}", BAD, input_dtype=pair[0], efeat_dtype=pair[1])
    for pair in ((FP32, FP32), (FP32, FP16), (FP32, BF16)):
        add(FORWARD, f"gate pair={pair}", LAUNCH, op=GATE, input_dtype=pair[0], efeat_dtype=pair[1])
    for pair in ((FP16, FP16), (BF16, BF16)):                 # the gate's gathered operand is grad_out: fp32 only
        add(FORWARD, f"gate pair={pair}", BAD, op=GATE, input_dtype=pair[0], efeat_dtype=pair[1])
    add(FORWARD, "copy ignores input_dtype", LAUNCH, op=COPY, input_dtype=7, efeat_dtype=FP16)
    # ---- the gradient for efeat: what each op reads is required, the rest may be NULL
    for p in ("indptr", "indices", "grad_out", "feat", "efeat", "output"):
        add(GRAD, f"{p}=NULL", BAD, **{p: NULL})
    add(GRAD, "op=4", BAD, op=COPY + 1)
    for op in (MUL, ADD, COPY):
        add(GRAD, f"op={op}", LAUNCH, op=op)
    add(GRAD, "mul efeat=NULL", LAUNCH, op=MUL, efeat=NULL)
    add(GRAD, "mul feat=NULL", BAD, op=MUL, feat=NULL)
    add(GRAD, "mul indices=NULL", BAD, op=MUL, indices=NULL)
    for op in (ADD, COPY):
        add(GRAD, f"op={op} indices=feat=efeat=NULL", LAUNCH, op=op, indices=NULL, feat=NULL, efeat=NULL)
        add(GRAD, f"op={op} grad_out=NULL", BAD, op=op, grad_out=NULL)
    for d in (-1, 3):
        add(GRAD, f"dtype={d}", BAD, dtype=d)
    for d in (FP16, BF16):
        add(GRAD, f"dtype={d}", LAUNCH, dtype=d)
        add(GRAD, f"dtype={d} embedding_dim=V+1", BAD, dtype=d, embedding_dim=9)
        add(GRAD, f"dtype={d} embedding_dim=4", BAD, dtype=d, embedding_dim=4)
    add(GRAD, "num_entries=0", OK, num_entries=0)
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
