"""Child process of tests/test_core_abi_host.py: every call of tests/core_abi_cases.py against libvoltrix_hip.so, on HOST buffers, in a
process that cannot see a device -- a call that slips past a missing check ends at the runtime's "no device", not in a kernel launch on
host pointers.  The parent hides the devices (HIP_VISIBLE_DEVICES=-1); this process asks the HIP runtime for its device count before the
first library call and makes none unless that count is zero (exit code 3).

    python core_abi_worker.py

A value goes through the binding's own argument types (``capi.SIGNATURES``): a Python float becomes the C float, seeds and offsets the
64-bit unsigned words, a threshold the 32-bit one.

Prints ``{"devices": n}`` first, then one JSON line ``{"id": ..., "rc": ...}`` per case as it returns (so that a crash names the case
it happened in: the first one without a line), then ``{"done": count}``.  No torch, no package import: voltrix/capi.py is loaded by path.
"""
import ctypes
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
EXIT_DEVICE_VISIBLE = 3
sys.path.insert(0, HERE)

import core_abi_cases as table  # noqa: E402

spec = importlib.util.spec_from_file_location("voltrix_capi_by_path", os.path.join(REPO, "voltrix-spmm_amd", "voltrix", "capi.py"))
capi = importlib.util.module_from_spec(spec)
spec.loader.exec_module(capi)


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


def call(lib, case):
    r = table.ROWS[case["name"]]
    argtypes = capi.SIGNATURES[case["name"]][1]
    assert len(argtypes) == len(r["params"]), case["name"]
    keep, base = [], {}
    for pname, role in r["params"]:
        if role.kind == "pointer":
            buf = ctypes.create_string_buffer(4096 + 16)
            keep.append(buf)
            base[pname] = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
            for i, v in enumerate(role.init or ()):
                ctypes.c_int.from_address(base[pname] + 4 * i).value = v
    assert not set(case["overrides"]) - {p for p, _ in r["params"]}, case["id"]
    rc = ctypes.c_int(-1)
    args = []
    for (pname, role), ctype in zip(r["params"], argtypes):
        value = case["overrides"].get(pname, role.value)
        if role.kind == "rc":
            args.append(ctypes.byref(rc))
        elif role.kind == "stream":
            args.append(None)
        elif role.kind == "pointer":
            if value is None:
                address = None
            elif value == table.SET:
                address = base[pname]
            elif value[0] == "off":
                address = base[pname] + value[1]
            else:
                assert value[0] == "same"
                address = base[value[1]]
            if ctype is not ctypes.c_void_p and address is not None:       # a typed host pointer (level_off_host)
                args.append(ctypes.cast(ctypes.c_void_p(address), ctype))
            else:
                args.append(address if address is None else ctypes.c_void_p(address))
        else:
            args.append(value)
    getattr(lib, case["name"])(*args)
    return rc.value


def main() -> int:
    lib = capi.lib()
    devices = visible_devices(lib)
    say({"devices": devices})
    if devices != 0:
        say({"refused": f"{devices} device(s) visible: no library call is made"})
        return EXIT_DEVICE_VISIBLE
    count = 0
    for case in table.cases():
        say({"id": case["id"], "rc": call(lib, case)})
        count += 1
    for name, args, _ in table.SIZE_FUNCTIONS:
        say({"id": f"{name}{args}", "rc": int(getattr(lib, name)(*args))})
        count += 1
    say({"done": count})
    return 0


if __name__ == "__main__":
    sys.exit(main())
