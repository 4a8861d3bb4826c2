"""Build-and-pick autotuner for JIT kernels.

Counterpart of the reference's voltrix/jit_kernels/tuner.py:42-168: every point of ``space`` is rendered
(``cpp_format`` -> ``generate``), built in parallel, run once for validity (non-zero return code = skipped;
here the kernels really set it), timed, and the fastest ``Runtime`` is memoised per ``(name, keys)``.
Round 4 -- the sweep is BOUNDED (the reference times 3 variants x 17 runs, tuner.py:135-141; rounds 2-3 here timed 44 tiles x
11 full-size launches: 39 s on the papers-like graph, 60 s on the power-law one):
  * candidates are timed on a SAMPLE of the work when the caller provides one (``sample_args``: the same kernels on a few
    contiguous window ranges of the handle, 1/16 of it) -- validity runs included;
  * the space is walked in STAGES when the caller provides ``stages`` (tile shapes first, each with its most robust schedule,
    then the schedules of the winning shape): <= 12 candidates instead of the cross product;
  * a wall-clock budget (``budget_s``: max(2 s, 20 x the estimated full step)) ends the sweep early with the best so far.
Differences from the reference, all deliberate:
  * builds run in a thread pool of hipcc subprocesses, not a forked ``mp.Pool`` (forking a process that has
    initialised HIP is not safe);
  * timing is HIP events on the launch stream (utils.GPU_bench), not kineto text scraping;
  * the winning point is also persisted in ``<cache dir>/tuned.json`` so that a later process builds/loads only
    that variant (the reference forgets it at exit, tuner.py:44,164).
"""
from __future__ import annotations

import copy
import fcntl
import json
import os
import time
from concurrent.futures import ThreadPoolExecutor
from typing import Any, Callable, Dict, Optional

from ..jit import build, cpp_format, generate
from ..jit.compiler import get_default_user_dir, parallel_compiles, put
from ..project import DEBUG_FLAG, PRINT_AUTOTUNE_FLAG


def _debug() -> bool:
    return bool(os.getenv(DEBUG_FLAG, None))


def _build_one(name, arg_defs, code, tuned_keys):
    try:
        return build(name, arg_defs, code), tuned_keys
    except Exception as exc:  # an illegal point of the space must not kill tuning (reference tuner.py:35-39)
        jit_tuner.stats["build_failures"] += 1   # ... but it must not go unseen either (tests assert zero)
        if _debug():
            print(f"JIT build of {name} {tuned_keys} failed: {exc}")
        return None, tuned_keys


class JITTuner:
    def __init__(self) -> None:
        self.tuned: Dict[Any, Any] = {}
        self.tuned_keys: Dict[Any, Dict] = {}
        # what this process has done so far (tests / bench.py): sweeps run, candidate kernels timed, choices taken from the
        # persisted exact key / from the persisted graph-statistics bucket; points that failed to build and candidates whose
        # validity launch returned nonzero (both dropped from the sweep: every point of the space should build and run)
        self.stats: Dict[str, Any] = {"sweeps": 0, "timed_candidates": 0, "stored_hits": 0, "bucket_hits": 0,
                                      "sweep_seconds": 0.0, "sweeps_cut_by_budget": 0, "full_size_checks": 0,
                                      "build_failures": 0, "illegal_candidates": 0}
        # signatures whose Runtime came from a persisted choice and has not run yet (no validation launch is made: the first
        # real launch is the validation -- ``forget`` + a sweep if it fails)
        self.unvalidated = set()
        # bumped whenever a memoised choice is dropped: launch plans built on a choice (jit_kernels/spmm.py) check it
        self.generation = 0

    # ---- persistent choices ------------------------------------------------------------------------------
    @staticmethod
    def _store_path() -> str:
        """The user's store of choices: ``$VOLTRIX_TUNED_STORE``, else ``tuned.json`` in the JIT cache directory."""
        return os.environ.get("VOLTRIX_TUNED_STORE") or os.path.join(get_default_user_dir(), "tuned.json")

    @staticmethod
    def _read(path: str) -> Dict[str, Dict]:
        try:
            with open(path, "r") as f:
                data = json.load(f)
            return data if isinstance(data, dict) else {}
        except (OSError, ValueError):
            return {}

    def _load_store(self) -> Dict[str, Dict]:
        """Shipped defaults (``tuned_defaults.json`` beside this file: graph-statistics BUCKET entries measured on MI355X,
        harness/collect_tuned.sh) under the user's own store, which wins."""
        store = self._read(os.path.join(os.path.dirname(os.path.abspath(__file__)), "tuned_defaults.json"))
        store.pop("_doc", None)
        if os.environ.get("VOLTRIX_TUNED_DEFAULTS", "1") in ("0", "off"):
            store = {}
        store.update(self._read(self._store_path()))
        return store

    def _save_choice(self, signature, tuned_keys, more_signatures=()) -> None:
        """Persist one choice under its exact key and any coarser keys, as ONE read-modify-write of the user's file under an
        exclusive lock (several ranks of one node finish their sweeps at the same time: an unlocked update loses entries)."""
        path = self._store_path()
        try:
            os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
            with open(path + ".lock", "w") as lock:
                fcntl.flock(lock, fcntl.LOCK_EX)
                try:
                    store = self._read(path)   # the user's file only: shipped defaults are never copied into it
                    for sig in (signature, *more_signatures):
                        store[f"{sig[0]}|{sig[1]}"] = tuned_keys
                    put(path, json.dumps(store, indent=1, sort_keys=True))
                finally:
                    fcntl.flock(lock, fcntl.LOCK_UN)
        except OSError:
            pass

    def forget(self, name: str, keys: Dict[str, Any]) -> None:
        """Drop the memoised choice for ``(name, keys)`` (its first launch failed): the next ``compile_and_tune`` sweeps."""
        sig = self._signature(name, keys)
        self.generation += 1
        self.tuned.pop(sig, None)
        self.tuned_keys.pop(sig, None)
        self.unvalidated.discard(sig)

    @staticmethod
    def _signature(name: str, keys: Dict[str, Any]):
        keys = {k: keys[k] for k in sorted(keys.keys())}
        return (name, f"{keys}")

    def is_tuned(self, name: str, keys: Dict[str, Any]) -> bool:
        """True when ``compile_and_tune(name, keys, ...)`` will not run a sweep (memoised in this process)."""
        return self._signature(name, keys) in self.tuned

    def tuned_point(self, name: str, keys: Dict[str, Any]) -> Dict:
        """The point of the space chosen for ``(name, keys)`` (after ``compile_and_tune``)."""
        return self.tuned_keys.get(self._signature(name, keys), {})

    # ---- main entry --------------------------------------------------------------------------------------
    def compile_and_tune(self, name: str, keys: Dict[str, Any], space: tuple, includes: tuple, arg_defs: tuple,
                         template: str, args: tuple, kernel_tag: Optional[str] = None,
                         bench: Optional[Callable] = None, bucket_keys: Optional[Callable[[], Any]] = None,
                         use_store: bool = True, sample_args: Optional[Callable[[], list]] = None,
                         stages: Optional[Callable] = None, budget_s: Optional[Callable[[float], float]] = None):
        """``bucket_keys`` (optional, called only when a sweep is about to run): a coarser key for the same choice -- the
        matrix tag replaced by a bucket of graph statistics.  The sweep's result is stored under
        both keys; a later process whose exact key has no entry (a new or untagged graph of the same shape class) takes the
        bucket's choice and runs no sweep: one build (a cache hit when the kernel exists on disk), no launch at all (the
        caller's first real launch validates it; ``use_store=False`` after such a launch failed).
        ``sample_args`` (called only when a sweep runs) -> ``(list of argument tuples, fraction)``: every candidate is run and
        timed on those launches instead of ``args`` (``fraction`` of the full work, for the budget).  ``stages(space, best,
        stage_no)`` -> the candidates of stage 0 (``best`` None) and of every later stage given the best point so far (an
        empty list ends the sweep); None = every point of ``space``.  ``budget_s(estimated full-size step in seconds)`` -> wall-clock cap of the sweep."""
        keys = {k: keys[k] for k in sorted(keys.keys())}
        signature = (name, f"{keys}")
        if signature in self.tuned:
            if _debug():
                print(f"Using cached JIT kernel {name} with keys {keys}")
            return self.tuned[signature]
        if _debug():
            print(f"Auto-tuning JIT kernel {name} with keys {keys}")
        assert args is not None
        space = (dict(),) if len(space) == 0 else tuple(space)

        def render(tuned_keys):
            full = copy.deepcopy(keys)
            full.update(tuned_keys)
            return generate(includes, arg_defs, cpp_format(template, full))

        # a choice persisted by an earlier process short-circuits the sweep: the exact key first, then the bucket
        bucket_signatures = []
        if len(space) > 1 and use_store:
            store = self._load_store()
            stored = store.get(f"{signature[0]}|{signature[1]}")
            hit = "stored_hits"
            if bucket_keys is not None and (stored is None or stored not in list(space)):
                bk = bucket_keys()      # one key, or several from the finest to the coarsest (the first that hits wins)
                for one in ([] if bk is None else (bk if isinstance(bk, (list, tuple)) else [bk])):
                    bucket_signatures.append(self._signature(name + "@bucket", one))
                for sig in bucket_signatures:
                    stored = store.get(f"{sig[0]}|{sig[1]}")
                    hit = "bucket_hits"
                    if stored is not None and stored in list(space):
                        break
            if stored is not None and stored in list(space):
                runtime, _ = _build_one(name, arg_defs, render(stored), stored)
                if runtime is not None:
                    self.tuned[signature], self.tuned_keys[signature] = runtime, stored
                    self.unvalidated.add(signature)
                    self.stats[hit] += 1
                    if _debug() or os.getenv(PRINT_AUTOTUNE_FLAG, None):
                        print(f"JIT kernel {name} with keys {keys}: persisted choice {stored} ({hit})")
                    return runtime
        if len(space) > 1:
            self.stats["sweeps"] += 1

        def build_all(points):
            workers = parallel_compiles(len(points))
            with ThreadPoolExecutor(max_workers=workers) as pool:
                futures = [pool.submit(_build_one, name, arg_defs, render(tk), tk) for tk in points]
                built = [f.result() for f in futures]
            return [(rt, tk) for rt, tk in built if rt is not None]

        t_sweep = time.perf_counter()
        launches, fraction = ([args], 1.0)
        if len(space) > 1 and sample_args is not None:
            launches, fraction = sample_args()

        def run_all(runtime):
            rc = 0
            for a in launches:
                rc = rc or runtime(*a)
            return rc

        best_runtime, best_time, best_keys = None, None, None
        deadline = None
        timed = []
        runtime_of = {}         # str(tuned keys) -> runtime of every timed candidate (the full-size decider below)
        stage_points = list(space) if (stages is None or len(space) <= 1) else list(stages(space, None))
        num_built = 0
        for stage_no in range(4):
            t_build = time.perf_counter()
            kernels = build_all(stage_points)
            if deadline is not None:     # the budget bounds TIMING: hipcc builds of a cold cache do not eat it (the same stages,
                deadline += time.perf_counter() - t_build    # hence the same choice, whether or not the kernels were on disk)
            num_built += len(kernels)
            for runtime, tuned_keys in kernels:
                if len(space) > 1:
                    if deadline is not None and time.perf_counter() > deadline and best_runtime is not None:
                        self.stats["sweeps_cut_by_budget"] += 1
                        break
                    if run_all(runtime) != 0:  # illegal kernel for these arguments (e.g. LDS budget, alignment)
                        self.stats["illegal_candidates"] += 1
                        if _debug():
                            print(f"Illegal JIT kernel {name} with keys {keys} and tuned keys {tuned_keys}")
                        continue
                    if bench is not None:
                        elapsed = bench(lambda: run_all(runtime))
                    else:
                        from ..utils import GPU_bench

                        elapsed = GPU_bench(lambda: run_all(runtime), iters=8, warmup=2, kernel_name=kernel_tag)
                    self.stats["timed_candidates"] += 1
                    timed.append((elapsed, tuned_keys))
                    runtime_of[str(tuned_keys)] = runtime
                    if deadline is None and budget_s is not None:   # the first timing prices the full-size step
                        deadline = t_sweep + budget_s(elapsed * 1e-3 / max(fraction, 1e-9))
                else:
                    elapsed = 0.0
                if best_time is None or elapsed < best_time:
                    best_runtime, best_time, best_keys = runtime, elapsed, tuned_keys
                if _debug():
                    print(f"Tuned JIT kernel {name} with keys {keys} and tuned keys {tuned_keys} has time {elapsed}")
            if stages is None or len(space) <= 1 or best_keys is None:
                break
            if deadline is not None and time.perf_counter() > deadline:
                break
            done = [tk for _, tk in timed]
            stage_points = [tk for tk in stages(space, best_keys, stage_no + 1) if tk not in done]
            if not stage_points:
                break
        # ---- full-size decider (round 6).  The candidates were ranked on a SAMPLE of the handle; on graphs whose operands live in HBM
        # the sample's ranking of the two or three best tiles is within its noise and the full-size steps are not (products-like,
        # relabelled: one process chose a tile of 3.32 ms, another one of 4.16 ms for the same handle).  Two or three finalists of the sample run
        # the WHOLE handle -- one warm-up + three timed launches each -- while the sweep's budget lasts; the faster one is the choice.
        if fraction < 0.5 and len(timed) >= 2 and best_keys is not None:
            import torch

            ranked = sorted(timed, key=lambda t: t[0])
            finalists = pick_finalists(timed, FINALISTS)
            full_ms = {}
            for tk in finalists:
                rt = runtime_of[str(tk)]
                est = (ranked[0][0] * 1e-3 / max(fraction, 1e-9)) * 4
                if len(full_ms) >= 2 and deadline is not None and time.perf_counter() + est > deadline + FINAL_GRACE_S:
                    break
                if rt(*args) != 0:
                    continue
                runs = []
                for _ in range(3):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    rt(*args)
                    b.record()
                    b.synchronize()
                    runs.append(a.elapsed_time(b))
                full_ms[str(tk)] = (sorted(runs)[1], tk, rt)
                self.stats["full_size_checks"] += 1
            if len(full_ms) >= 2:
                best_time, best_keys, best_runtime = min(full_ms.values(), key=lambda v: v[0])
                if _debug() or os.getenv(PRINT_AUTOTUNE_FLAG, None):
                    print(f"JIT kernel {name}: full-size decider {[(str(v[1]), round(v[0], 4)) for v in full_ms.values()]}")
        kernels = [None] * num_built
        self.stats["sweep_seconds"] += time.perf_counter() - t_sweep if len(space) > 1 else 0.0
        assert best_runtime is not None, f"Failed to tune JIT kernel {name} with keys {keys}"

        if _debug() or os.getenv(PRINT_AUTOTUNE_FLAG, None):
            print(f"JIT kernel {name}[in {len(kernels)}/{len(space)}] with keys {keys} has tuned keys {best_keys} "
                  f"and time {best_time:.4f}ms")
        self.tuned[signature], self.tuned_keys[signature] = best_runtime, best_keys
        if len(space) > 1:
            self._save_choice(signature, best_keys, bucket_signatures)
        return best_runtime


def pick_finalists(timed, limit):
    """The candidates of a sample-timed sweep that run the whole handle: the sample's best, then the best of every OTHER schedule
    (what a sample misjudges is the schedule -- how a slice's windows balance says little about the whole handle's; shape and
    depth it ranks reliably), then the runners-up; ``timed`` = [(ms on the sample, tuned keys)]."""
    ranked = [tk for _, tk in sorted(timed, key=lambda t: t[0])]
    out = ranked[:1]
    for tk in ranked[1:]:
        if all(tk.get("SCHED") != f.get("SCHED") for f in out):
            out.append(tk)
    out += [tk for tk in ranked[1:] if tk not in out]
    return out[:limit]


FINALISTS = 3            # candidates of the sample ranking that run the whole handle before the choice is made (two always, the
FINAL_GRACE_S = 0.5      # third while the sweep's budget + this grace lasts)

jit_tuner = JITTuner()
