"""Cases of tests/test_gpu_tile_matrix.py, shared with its CPU checks (tests/test_host_logic.py): the two adversarial graphs and
the (tile point, feature width) pairs the tuner can pick, enumerated with ``tile_space`` itself."""
import json
import os

import numpy as np

from voltrix.jit_kernels import spmm as spmm_mod

W16 = (8, 40, 128, 264)      # 16-bit operands: 264 = three 128-column slabs and a tail of 8
W32 = (4, 36, 64, 132)       # fp32 operands
MODES = ("none", "stream", "default")
# the flag sets spmm_kernel passes to tile_space (name -> keyword arguments)
FLAG_SETS = {"plain": {}, "weighted": {"weighted": True}, "max_lds": {"max_lds": spmm_mod.TWO_LEVEL_LDS_BUDGET},
             "no_stream": {"stream_ok": False}, "deep": {"shallow_ok": False}}
KINDS = {"f16": (2, False), "bf16": (2, True), "f32": (4, False)}

G1_N = 16 * 640 + 13
G2_N = 16 * 1200 + 1


def point_key(point):
    return tuple(sorted(point.items()))


def kind_of(point):
    return "f32" if point["EB"] == 4 else ("bf16" if point["BF16"] else "f16")


def shipped_defaults():
    path = os.path.join(os.path.dirname(spmm_mod.__file__), "tuned_defaults.json")
    with open(path) as f:
        store = json.load(f)
    store.pop("_doc", None)
    return store


def enumerate_points():
    """{point key: {width: set of flag-set names that offer the point at that width}} over every mode, width and flag set; the
    points of ``tuned_defaults.json`` join at the widest width of their operand type when no listed width offers them."""
    out = {}
    for kind, (eb, bf16) in KINDS.items():
        for width in (W16 if eb == 2 else W32):
            for mode in MODES:
                with spmm_mod.tune_space(mode):
                    for flag, kw in FLAG_SETS.items():
                        if flag == "weighted" and eb != 2:
                            continue
                        for p in spmm_mod.tile_space(width, eb, bf16, **kw):
                            out.setdefault(point_key(p), {}).setdefault(width, set()).add(flag)
    for point in shipped_defaults().values():
        if point_key(point) not in out:
            width = max(W16 if point["EB"] == 2 else W32)
            out[point_key(point)] = {width: {"weighted" if point["WEIGHTED"] else "plain"}}
    return out


def case_id(point, width, slab_policy=None):
    p = dict(point)
    name = f"{kind_of(p)}{'w' if p['WEIGHTED'] else ''}-FS{p['FS']}-D{p['DEPTH']}-W{p['WAVES']}-S{p['SCHED']}-F{width}"
    return name if slab_policy is None else f"{name}-P{slab_policy}"


def cases():
    """[(id, point dict, width, flag-set names, SLAB_POLICY or None)]: multi-slab widths (wider than the tile's slab) run under
    both slab policies."""
    out = []
    for key, widths in sorted(enumerate_points().items()):
        point = dict(key)
        for width, flags in sorted(widths.items()):
            policies = (0, 1) if width > point["FS"] else (None,)
            for policy in policies:
                out.append((case_id(point, width, policy), point, width, frozenset(flags), policy))
    return out


def full_only_shapes():
    """(FS, DEPTH, WAVES, EB) of ``VOLTRIX_TUNE_SPACE=full`` at the widest widths that no other mode offers at any width."""
    others = {(dict(k)["FS"], dict(k)["DEPTH"], dict(k)["WAVES"], dict(k)["EB"]) for k in enumerate_points()}
    shapes = set()
    with spmm_mod.tune_space("full"):
        for eb, width in ((2, max(W16)), (4, max(W32))):
            for p in spmm_mod.tile_space(width, eb):
                shapes.add((p["FS"], p["DEPTH"], p["WAVES"], p["EB"]))
    return sorted(shapes - others)


def _csr(rows, n):
    indptr = np.zeros(n + 1, np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    indices = np.concatenate([np.asarray(r, np.int64) for r in rows] + [np.zeros(0, np.int64)])
    return indptr.astype(np.int32), indices.astype(np.int32)


def graph_cuts(seed=0):
    """G1: N = 16 * 640 + 13.  Windows of 1-3 TC blocks (banded rows of degree 0-2); runs of empty windows, window 0 and the
    last, partial window among them; a hub row (degree 2000 .. N) in the window on either side of each of the seven inner
    boundaries of eight equal window ranges and in the last full window (that one of degree N: every column is gathered);
    one window whose 16 rows are all hubs."""
    rng = np.random.default_rng(seed)
    n = G1_N
    nw = (n + 15) // 16
    empty = {0, 1, 2, 300, 301, 302, 303, 304, 520, 521, nw - 1}
    rows = []
    for r in range(n):
        if r // 16 in empty:
            rows.append([])
            continue
        deg = int(rng.choice(3, p=(0.3, 0.5, 0.2)))
        lo, hi = max(0, r - 8), min(n, r + 9)
        rows.append(np.sort(rng.choice(np.arange(lo, hi), deg, replace=False)))
    wpx = -(-nw // 8)
    hub_windows = [wpx * k - (k % 2) for k in range(1, 8)] + [nw - 2]
    for w in hub_windows:
        r = 16 * w + int(rng.integers(0, 16))
        deg = n if w == nw - 2 else int(rng.integers(2000, n + 1))
        rows[r] = np.sort(rng.choice(n, deg, replace=False))
    all_hubs = 4 * wpx + wpx // 2
    for r in range(16 * all_hubs, 16 * all_hubs + 16):
        rows[r] = np.sort(rng.choice(n, int(rng.integers(2000, 4000)), replace=False))
    indptr, indices = _csr(rows, n)
    return indptr, indices, n


def graph_short(seed=1):
    """G2: N = 16 * 1200 + 1, uniform columns of degree 0-4 (2-6 TC blocks per window); windows 600-602 empty; the last
    window's only row has the single column N - 1."""
    rng = np.random.default_rng(seed)
    n = G2_N
    rows = []
    for r in range(n - 1):
        if r // 16 in (600, 601, 602):
            rows.append([])
            continue
        rows.append(np.sort(rng.choice(n, int(rng.integers(0, 5)), replace=False)))
    rows.append([n - 1])
    indptr, indices = _csr(rows, n)
    return indptr, indices, n


GRAPHS = {"cuts": graph_cuts, "short": graph_short}
