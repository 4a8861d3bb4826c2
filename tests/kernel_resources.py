"""The compiler's own resource report of a set of kernels: the source is compiled for gfx950 with
``-Rpass-analysis=kernel-resource-usage`` (hipcc cross-compiles: no GPU), and the remarks of the kernels whose name holds one of
``keys`` are parsed.  The per-operator host tests keep their own ``SOURCE`` and their own assertions (kernel counts, zeros)."""
import os
import re
import subprocess

from conftest import REPO

INCLUDE = os.path.join(REPO, "voltrix-spmm_amd", "voltrix", "include")
FIELDS = (r"ScratchSize \[bytes/lane\]", "SGPRs Spill", "VGPRs Spill", r"LDS Size \[bytes/block\]")


def resource_usage(source, workdir, stem, keys):
    """``({kernel: (scratch bytes per lane, spilled SGPRs, spilled VGPRs, static LDS bytes per block)}, report)`` of the kernels of
    ``source`` whose (mangled) name holds one of ``keys``; ``report``: their remark lines, each from the header's path on (what the
    ``resource_usage.txt`` files under profiles/ hold)."""
    src = os.path.join(str(workdir), stem + ".hip")
    with open(src, "w") as f:
        f.write(source)
    run = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", INCLUDE,
                          "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.path.join(str(workdir), stem + ".o")],
                         capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-3000:]
    usage = {}
    for block in run.stderr.split("remark: Function Name: ")[1:]:
        name = block.split(" ")[0].strip()
        if any(key in name for key in keys):
            usage[name] = tuple(int(re.search(field + r": (\d+)", block).group(1)) for field in FIELDS)
    report, wanted = [], False
    for line in run.stderr.splitlines():
        if "remark:" not in line:
            continue
        if "remark: Function Name: " in line:
            wanted = line.split("remark: Function Name: ")[1].split(" ")[0].strip() in usage
        if wanted:
            report.append(line.split(INCLUDE + os.sep, 1)[-1])
    return usage, "\n".join(report) + "\n"
