"""Child process of tests/test_spmm_multi_host.py: the host-side argument contract of ``voltrix_spmm_multi_csr`` and
``voltrix_spmm_multi_backward_csr`` on 16-byte-aligned HOST buffers, in a process that cannot see a device -- a call that slips past a
missing check ends at the runtime's "no device" (2), not in a kernel launch on host pointers.  The protocol of
tests/spmm_fp8_abi_worker.py: the parent hides the devices (HIP_VISIBLE_DEVICES=-1); this process asks the HIP runtime for its device
count before the first library call and makes none unless that count is zero (exit code 3).

    python spmm_multi_abi_worker.py

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

FORWARD = "voltrix_spmm_multi_csr"
BACKWARD = "voltrix_spmm_multi_backward_csr"
SYMBOLS = (FORWARD, BACKWARD)
SLOTS = ("slot_sum", "slot_mean", "slot_max", "slot_min", "slot_var", "slot_std")
# parameter order of the header; the baseline of each symbol is a valid call with everything on (answered with "no device")
PARAMS = {
    FORWARD: [("indptr", SET), ("indices", SET), ("num_rows", 4), ("num_entries", 8), ("embedding_dim", 24), ("input", SET),
              ("dtype", FP32), ("slot_sum", 0), ("slot_mean", 1), ("slot_max", 2), ("slot_min", 3), ("slot_var", 4), ("slot_std", 5),
              ("num_slots", 6), ("eps", 1e-5), ("output", SET), ("argmax", SET), ("argmin", SET), ("stream", NULL)],
    BACKWARD: [("t_indptr", SET), ("t_indices", SET), ("t_order", SET), ("num_cols", 4), ("num_entries", 8), ("embedding_dim", 24),
               ("x", SET), ("u", SET), ("w", SET), ("mean", SET), ("mean_ld", 48), ("g_max", SET), ("argmax", SET), ("g_min", SET),
               ("argmin", SET), ("output", SET), ("stream", NULL)],
}
ROWS = {FORWARD: "num_rows", BACKWARD: "num_cols"}
FOUR = {FORWARD: ("indptr", "indices"), BACKWARD: ("t_indptr", "t_indices", "t_order")}                 # 4-byte loads
SIXTEEN = {FORWARD: ("input", "output", "argmax", "argmin"),
           BACKWARD: ("x", "u", "w", "mean", "g_max", "argmax", "g_min", "argmin", "output")}
POINTERS = {s: FOUR[s] + SIXTEEN[s] for s in SYMBOLS}
# what NULL means per pointer: refused, or another valid call
NULL_ANSWER = {
    FORWARD: {"indptr": BAD, "indices": BAD, "input": BAD, "output": BAD, "argmax": LAUNCH, "argmin": LAUNCH},
    # with entries, t_indices is required and so is t_order beside a routed gradient; a group given in part is refused; u stands alone
    BACKWARD: {"t_indptr": BAD, "t_indices": BAD, "t_order": BAD, "output": BAD, "u": LAUNCH, "x": BAD, "w": BAD, "mean": BAD,
               "g_max": BAD, "argmax": BAD, "g_min": BAD, "argmin": BAD},
}


def cases():
    out = []

    def add(symbol, what, expected, **overrides):
        out.append((f"{symbol}::{what}", symbol, overrides, expected))

    for symbol in SYMBOLS:
        add(symbol, "baseline", LAUNCH)
        for p in POINTERS[symbol]:
            add(symbol, f"{p}=NULL", NULL_ANSWER[symbol][p], **{p: NULL})
        for p in FOUR[symbol]:
            add(symbol, f"{p}+2", BAD, **{p: ("off", 2)})
        for p in SIXTEEN[symbol]:
            for off in (4, 8):
                add(symbol, f"{p}+{off}", BAD, **{p: ("off", off)})
        add(symbol, "rows=-1", BAD, **{ROWS[symbol]: -1})
        add(symbol, "embedding_dim=-1", BAD, embedding_dim=-1)
        add(symbol, "num_entries=-1", BAD, num_entries=-1)
        add(symbol, "num_entries=2^31", BAD, num_entries=2 ** 31)
        add(symbol, "num_entries=2^31-1", LAUNCH, num_entries=2 ** 31 - 1)
        add(symbol, "num_entries=0", LAUNCH, num_entries=0)
        add(symbol, "num_entries=-1 rows=0", BAD, num_entries=-1, **{ROWS[symbol]: 0})     # sizes come before "nothing to do"
        # nothing to do: no launch, and no pointer is looked at
        add(symbol, "rows=0", OK, **{ROWS[symbol]: 0})
        add(symbol, "embedding_dim=0", OK, embedding_dim=0)
    everything = {p: NULL for p in POINTERS[FORWARD]}
    add(FORWARD, "rows=0 every pointer NULL", OK, num_rows=0, **everything)
    add(FORWARD, "embedding_dim=0 every pointer NULL", OK, embedding_dim=0, **everything)
    add(BACKWARD, "rows=0 required pointers NULL", OK, num_cols=0, t_indptr=NULL, t_indices=NULL, t_order=NULL, output=NULL)
    # the forward: the width in 16-byte pieces, the type
    for width in (1, 2, 6, 25):
        add(FORWARD, f"embedding_dim={width}", BAD, embedding_dim=width)
    add(FORWARD, "embedding_dim=12 fp16", BAD, embedding_dim=12, dtype=FP16)
    add(FORWARD, "embedding_dim=12 bf16", BAD, embedding_dim=12, dtype=BF16)
    add(FORWARD, "embedding_dim=25 rows=0", BAD, embedding_dim=25, num_rows=0)
    for d in (FP16, BF16):
        add(FORWARD, f"dtype={d}", LAUNCH, dtype=d)
    for d in (-1, 3):
        add(FORWARD, f"dtype={d}", BAD, dtype=d)
    add(FORWARD, "embedding_dim=4", LAUNCH, embedding_dim=4)
    add(FORWARD, "embedding_dim=260", LAUNCH, embedding_dim=260)
    # the slots: in range, no clash, every slot filled, the args only beside their selection
    for s in SLOTS:
        add(FORWARD, f"{s}=6", BAD, **{s: 6})
        add(FORWARD, f"{s}=-2", BAD, **{s: -2})
    for i, s in enumerate(SLOTS):
        add(FORWARD, f"{s} clashes", BAD, **{s: (i + 1) % 6})
    add(FORWARD, "a slot nobody fills", BAD, slot_sum=-1)
    add(FORWARD, "num_slots=0", BAD, num_slots=0)
    add(FORWARD, "num_slots=7", BAD, num_slots=7)
    add(FORWARD, "num_slots=-1", BAD, num_slots=-1)
    none = {s: -1 for s in SLOTS}
    add(FORWARD, "nothing stored", BAD, **none, num_slots=0, argmax=NULL, argmin=NULL)
    add(FORWARD, "pna", LAUNCH, **{**none, "slot_mean": 0, "slot_max": 1, "slot_min": 2, "slot_std": 3}, num_slots=4)
    add(FORWARD, "sum alone", LAUNCH, **{**none, "slot_sum": 0}, num_slots=1, argmax=NULL, argmin=NULL)
    add(FORWARD, "std alone", LAUNCH, **{**none, "slot_std": 0}, num_slots=1, argmax=NULL, argmin=NULL)
    add(FORWARD, "reversed order", LAUNCH, **{s: 5 - i for i, s in enumerate(SLOTS)})
    add(FORWARD, "argmax without max", BAD, **{**none, "slot_min": 0}, num_slots=1, argmin=NULL)
    add(FORWARD, "argmin without min", BAD, **{**none, "slot_max": 0}, num_slots=1, argmax=NULL)
    add(FORWARD, "args without selection", BAD, **{**none, "slot_mean": 0}, num_slots=1)
    add(FORWARD, "argmin alone beside min", LAUNCH, **{**none, "slot_min": 0}, num_slots=1, argmax=NULL)
    # eps: looked at where std is stored, and only there
    for name, eps in (("0", 0.0), ("-1", -1.0), ("inf", float("inf")), ("nan", float("nan"))):
        add(FORWARD, f"eps={name}", BAD, eps=eps)
        add(FORWARD, f"eps={name} rows=0", BAD, eps=eps, num_rows=0)
        add(FORWARD, f"eps={name} without std", LAUNCH, eps=eps, slot_std=-1, num_slots=5)
    add(FORWARD, "eps=1e-30", LAUNCH, eps=1e-30)
    # the backward: 4 features per lane, whole groups, the stride of mean
    for width in (1, 2, 6, 25):
        add(BACKWARD, f"embedding_dim={width}", BAD, embedding_dim=width, mean_ld=width)
    add(BACKWARD, "embedding_dim=25 rows=0", BAD, embedding_dim=25, num_cols=0)
    add(BACKWARD, "embedding_dim=4", LAUNCH, embedding_dim=4)
    add(BACKWARD, "mean_ld<embedding_dim", BAD, mean_ld=20)
    add(BACKWARD, "mean_ld=26", BAD, mean_ld=26)
    add(BACKWARD, "mean_ld=-4", BAD, mean_ld=-4)
    add(BACKWARD, "mean_ld=embedding_dim", LAUNCH, mean_ld=24)
    add(BACKWARD, "mean_ld unused without w", LAUNCH, mean_ld=-4, x=NULL, w=NULL, mean=NULL)
    sel = {"g_max": NULL, "argmax": NULL, "g_min": NULL, "argmin": NULL}
    mom = {"x": NULL, "w": NULL, "mean": NULL}
    add(BACKWARD, "no group", BAD, u=NULL, **sel, **mom)
    add(BACKWARD, "u alone", LAUNCH, **sel, **mom)
    add(BACKWARD, "u alone without t_order", LAUNCH, t_order=NULL, **sel, **mom)
    add(BACKWARD, "moments alone", LAUNCH, u=NULL, **sel)
    add(BACKWARD, "max alone", LAUNCH, u=NULL, g_min=NULL, argmin=NULL, **mom)
    add(BACKWARD, "min alone", LAUNCH, u=NULL, g_max=NULL, argmax=NULL, **mom)
    add(BACKWARD, "selections alone", LAUNCH, u=NULL, **mom)
    add(BACKWARD, "num_entries=0 without t_indices and t_order", LAUNCH, num_entries=0, t_indices=NULL, t_order=NULL)
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
