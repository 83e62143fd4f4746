#!/usr/bin/env python3
"""Headline benchmark: DRT fits/sec, 256 freq x 512 tau, batched (BASELINE.json), one process per GPU.

  python bench.py --gpus N --steps K --warmup W [--config auto|c3|c4]
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
      bench.py --gpus N --steps K --warmup W

Workloads (`--config`; default `auto`: `value` = c4 for EVERY N -- the workload BASELINE.json's metric is quoted on at
1 / 2 / 4 / 8 GPUs, strong scaling, K steps = K whole maps with upload, fit, llh / rss, download and the gather inside -- and,
with `--full`, the c3 legs (inputs resident / streamed, one plan in flight for the kernel's roofline figures) run beside it on
min(K, 8) steps and are reported as `value_resident`, `value_streamed`, `single_stream`, `single_caller` in the same line):
  c3  BASELINE configs[2]: `--batch` (1024) synthetic 2-ZARC spectra per GPU, shared 256-point frequency grid, 512-point
      tau grid.  A step = one full QPHB fit (DRT._qphb_fit_core: scaling, initial-weights QP, hyper-parameter loop to
      convergence, final q) of the batch, inputs resident in HBM when the timed region starts.  Weak scaling over ranks.
  c4  BASELINE configs[3]: ONE map of `--total` (10 000) spectra sharded over the ranks (interleaved shards; every rank
      fits its share on one plan that cuts it into side-by-side ranges, or on `--inflight` plans), a step = upload + fit + download on every rank + one gather of the
      results on rank 0, all inside the timed region.  Strong scaling.
Rank 0 prints ONE JSON line.  `value` is always whole-job fits per second.

A plain run measures the headline alone: for `auto`, set-up, W warm-up maps (at least one: it builds the plans), K timed maps
and the result line (`metric`, `value`, `unit`, `higher_is_better`, `dtype`, `ms_per_step` = one timed map, the workload);
for `c3` / `c4`, their first timed leg alone.  `--full` adds everything else the line has held: the c3 legs beside the map,
the rooflines and phase split, the single-spectrum and configs[4] timings, the matrix-build roofline and the CPU baselines
(the `--no-*` options switch single legs of a `--full` run off).
`--dump-outputs DIR` writes, after the timed steps, what the headline's last step returned to its caller as DIR/<name>.npy
(float64; integer and boolean fields converted, at most 64 MB: a larger output is cut to a fixed, seeded sample of its
rows, listed in DIR/rows.npy).  The inputs are seeded: the same arguments give the same inputs in every run.
"""
import argparse
import hashlib
import json
import os
import re
import sys
import time

# One BLAS / OpenMP thread per process, fixed BEFORE numpy / scipy load their BLAS: the CPU legs are "1 core" and "one
# single-threaded worker process per core"; a BLAS pool sized after the host's 256 cpus inside each of 256 forked workers is
# what made round 2's all-cores figure meaningless.  (The GPU path does not use host BLAS threads.)
for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS", "NUMEXPR_NUM_THREADS", "VECLIB_MAXIMUM_THREADS"):
    os.environ[_v] = "1"

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8 TB/s spec (6.3 TB/s achievable)
FP64_MFMA_PEAK_TFLOPS = 78.6   # vendor dense FP64 matrix peak (the guide lists no FP64 row)
QP_KERNEL = "qp_kernel_resident"          # as rocprofv3 prints it (hipdrt::qp_kernel_resident(hipdrt::QpArgs, int))


def qp_algorithmic_flop(n, qp_iters_total, n_qp):
    """per IPM iteration one Cholesky n^3/3 + two KKT solves of 2 n^2 each; every QP adds the start-point
    factorisation with one solve."""
    fact = (qp_iters_total + n_qp) * (n ** 3 / 3.0)
    solves = (2 * qp_iters_total + n_qp) * (2.0 * n * n)
    return fact + solves


def _code_only(name, text):
    """source text without comments and with runs of white space collapsed: the stamp below should follow the CODE, not a
    reworded comment (string literals in these sources hold no comment markers)"""
    if name == "Makefile":
        text = re.sub(r"#[^\n]*", "", text)
    else:
        text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
        text = re.sub(r"//[^\n]*", "", text)
    return re.sub(r"\s+", " ", text).strip()


def source_hash():
    """sha256 over the library's sources (code only: comments and white space do not count): stamps PMC traffic figures
    (profiles/qp_traffic.json) with the code they were measured on -- a figure from other sources is reported as null, not
    silently carried along."""
    h = hashlib.sha256()
    src = os.path.join(ROOT, "hybrid-drt_amd", "csrc")
    for name in sorted(os.listdir(src)):
        if name.endswith((".hip", ".hpp")) or name == "Makefile":
            with open(os.path.join(src, name), "r", encoding="utf-8", errors="replace") as f:
                h.update(name.encode())
                h.update(_code_only(name, f.read()).encode())
    with open(os.path.join(ROOT, "include", "hipdrt.h"), "r", encoding="utf-8", errors="replace") as f:
        h.update(_code_only("hipdrt.h", f.read()).encode())
    return h.hexdigest()[:16]


# ---- CPU baseline (the oracle = CPU restatement, used here as the thing timed beside the GPU; checker otherwise) --------
_POOL = {}


def _blas_threads():
    """what the loaded BLAS libraries say about their thread pools (threadpoolctl), as a short string for the sample text"""
    try:
        from threadpoolctl import threadpool_info
        return ", ".join(f"{d.get('internal_api', d.get('user_api'))}:{d.get('num_threads')}" for d in threadpool_info()) or "none loaded"
    except Exception as e:      # pragma: no cover
        return f"threadpoolctl unavailable ({e!r})"


def _pool_init(freq, tau, z):
    if "drt" in _POOL:              # forked worker: the parent's prepared oracle (and its 1-thread BLAS) came along
        return
    from oracle import drt_oracle as orc
    drt = orc.OracleDRT(fixed_basis_tau=tau)
    drt.prepare(freq)
    _POOL.update(drt=drt, freq=freq, z=z)


def _pool_work(args):
    first, stride, budget = args
    drt, freq, z = _POOL["drt"], _POOL["freq"], _POOL["z"]
    done, t0, c0, i = 0, time.perf_counter(), time.process_time(), first
    while time.perf_counter() - t0 < budget:
        drt.fit_eis(freq, z[i % len(z)], structure='fast')
        done += 1
        i += stride
    # (CPU seconds this worker was actually given, next to its wall time: a quota or an oversubscribed host shows up here)
    return done, time.perf_counter() - t0, _blas_threads(), time.process_time() - c0


def cgroup_cpu_limit():
    """CPU bandwidth limit of this container in cores (cgroup v2 cpu.max or v1 cfs quota), or None when unlimited / unknown"""
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()
        return None if q == "max" else float(q) / float(p)
    except Exception:
        pass
    try:
        q = float(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
        p = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        return None if q <= 0 else q / p
    except Exception:
        return None


def host_cores():
    """(physical cores, logical cpus) of this host from /proc/cpuinfo; physical falls back to logical"""
    logical = os.cpu_count() or 1
    try:
        pairs, phys, core = set(), None, None
        for line in open("/proc/cpuinfo"):
            if line.startswith("physical id"):
                phys = line.split(":")[1].strip()
            elif line.startswith("core id"):
                core = line.split(":")[1].strip()
            elif not line.strip():
                if phys is not None and core is not None:
                    pairs.add((phys, core))
                phys = core = None
        if phys is not None and core is not None:
            pairs.add((phys, core))
        physical = len(pairs) or logical
    except Exception:           # pragma: no cover
        physical = logical
    try:
        logical = min(logical, len(os.sched_getaffinity(0)))
    except Exception:           # pragma: no cover
        pass
    return min(physical, logical), logical


def cpu_baseline(freq, tau, z, seconds_budget=15.0, ref_structure_budget=8.0, procs=None, pool_budget=6.0):
    """The oracle timed on this host BEFORE the GPU is touched (the pool forks): (i) one process, one BLAS thread;
    (ii) the whole host: process pools over spectra, one single-threaded worker each, swept over
    {physical cores / 2, physical cores, logical cpus} workers -- the best is reported with its count and every point of
    the sweep is listed; (iii) 'reference_structure' mirrors the reference's own dense diag products (the O(n^3) work per
    outer iteration that hybrid-drt itself does) on a smaller sample, one process."""
    import multiprocessing as mp
    _pool_init(freq, tau, z)
    drt = _POOL["drt"]

    def timed(structure, budget):
        done, t0 = 0, time.perf_counter()
        while done < len(z):
            drt.fit_eis(freq, z[done], structure=structure)
            done += 1
            if time.perf_counter() - t0 > budget:
                break
        return done, time.perf_counter() - t0

    done, dt = timed('fast', seconds_budget)
    rdone, rdt = timed('reference', ref_structure_budget)
    one_core = done / dt
    physical, logical = host_cores()
    quota = cgroup_cpu_limit()                       # CPU bandwidth this container may use, in cores (None = no limit)
    if procs:
        counts = [min(procs, logical)]
    elif quota and quota < physical:
        # a container with a CPU quota: more runnable workers than the quota only take turns -- sweep around the quota
        q = max(1, int(round(quota)))
        counts = sorted({max(1, q // 2), q, min(2 * q, logical), min(4 * q, logical)})
    else:
        counts = sorted({min(8, logical), min(32, logical), max(1, physical // 2), physical, logical})
    sweep, allc = [], None
    ctx = mp.get_context("fork")            # nothing GPU-side exists yet in this process; children never touch it
    for n_workers in counts:
        try:
            t0 = time.perf_counter()
            with ctx.Pool(n_workers, initializer=_pool_init, initargs=(freq, tau, z)) as pool:
                t_up = time.perf_counter() - t0
                parts = pool.map(_pool_work, [(i, n_workers, pool_budget) for i in range(n_workers)], chunksize=1)
            fits = sum(p[0] for p in parts)
            wall = max(p[1] for p in parts)
            sweep.append(dict(workers=n_workers, value=fits / wall, fits=fits, seconds=wall, pool_startup_s=t_up,
                              per_worker_vs_one_core=fits / wall / n_workers / one_core,
                              cpu_seconds_over_wall=sum(p[3] for p in parts) / sum(p[1] for p in parts),
                              worker_blas_threads=sorted({p[2] for p in parts})))
        except Exception as e:          # noqa: BLE001 -- a box that cannot fork that many workers still reports the rest
            sweep.append(dict(workers=n_workers, value=None, error=repr(e)))
    good = [s_ for s_ in sweep if s_.get("value")]
    if good:
        best = max(good, key=lambda s_: s_["value"])
        eff_cores = min(best["workers"], physical, quota) if quota else min(best["workers"], physical)
        allc = dict(value=best["value"], unit="fits/s", cores=best["workers"], kind="port", cores_available=eff_cores,
                    physical_cores=physical, logical_cpus=logical, cgroup_cpu_limit=quota, sweep=sweep,
                    efficiency_vs_cores=best["value"] / (eff_cores * one_core),
                    sample=f"{best['fits']} fits of the batch's spectra in {best['seconds']:.1f} s: {best['workers']} forked worker "
                           f"processes, BLAS threads per worker {best['worker_blas_threads']} (OMP/OPENBLAS/MKL_NUM_THREADS=1 set "
                           f"before numpy was imported), every worker looping over its own stride of the batch; host has "
                           f"{physical} physical cores / {logical} logical cpus, cgroup CPU limit {quota} cores (`cores_available` = what "
                           f"the best pool could actually use; `efficiency_vs_cores` is against that); pool start-up not counted; per sweep point "
                           f"`cpu_seconds_over_wall` = CPU time the workers were given / their wall time (1.0 = every worker had "
                           f"a core to itself the whole time: then the loss against workers x the 1-core figure is contention "
                           f"for caches and memory bandwidth -- a fit streams its 2 MB P and L through several O(n^2) numpy passes "
                           f"per interior-point iteration --, not scheduling)")
    else:
        allc = dict(value=None, unit="fits/s", cores=0, kind="port", sweep=sweep, sample="every process pool failed")
    return dict(value=one_core, unit="fits/s", cores=1, kind="port",
                sample=f"first {done} of the batch's spectra (256x512, full QPHB loop), oracle/drt_oracle.py "
                       f"structure='fast', 1 process, BLAS threads {_blas_threads()}, {dt:.1f} s",
                all_cores=allc,
                reference_structure=dict(value=rdone / rdt, unit="fits/s", cores=1,
                                         sample=f"first {rdone} spectra, structure='reference' (the reference's dense "
                                                f"diag products restated one-for-one), 1 BLAS thread, {rdt:.1f} s"))


def self_launch(n):
    """`python bench.py --gpus N` without a launcher: N child processes of this very command line, one per rank, with
    RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT set (what torch.distributed.run would set); rank 0's stdout
    is passed through (the ONE JSON line), the other ranks' output goes to stderr.  Returns the exit code."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=None if r == 0 else sys.stderr))
    codes = [None] * n
    try:
        while any(c is None for c in codes):
            for r, pr in enumerate(procs):
                if codes[r] is None and pr.poll() is not None:
                    codes[r] = pr.returncode
                    if codes[r] != 0:                # a dead rank leaves the others waiting in a collective
                        for other in procs:
                            if other.poll() is None:
                                other.terminate()
            time.sleep(0.05)
    finally:
        for pr in procs:
            if pr.poll() is None:
                pr.kill()
    bad = [(r, c) for r, c in enumerate(codes) if c != 0]
    if bad:
        print(f"bench.py: ranks exited non-zero: {bad}", file=sys.stderr)
    return 1 if bad else 0


DUMP_LIMIT_BYTES = 64 << 20


def map_outputs(got):
    """the triple mapping.fit_observations_sharded returns on rank 0, as one flat dict of arrays"""
    obs_x, obs_special, res = got
    outputs = {"obs_x": obs_x}
    outputs.update({f"special_{k}": v for k, v in obs_special.items()})
    outputs.update({k: v for k, v in res.items() if k != "obs_fit_errors"})
    return outputs


def dump_outputs(dirname, outputs):
    """--dump-outputs: every numeric array of `outputs` as DIR/<name>.npy in float64 (complex as <name>_real / <name>_imag);
    dicts (timings) and non-numeric fields are left out.  Above DUMP_LIMIT_BYTES the arrays whose first axis is the batch
    keep a fixed, seeded sample of its rows (DIR/rows.npy), the others are written whole."""
    arrays = {}
    for name, v in outputs.items():
        if isinstance(v, dict):
            continue
        a = np.asarray(v)
        if a.dtype == object or a.dtype.kind not in "biufc":
            continue
        if a.dtype.kind == "c":
            arrays[name + "_real"], arrays[name + "_imag"] = a.real.astype(np.float64), a.imag.astype(np.float64)
        else:
            arrays[name] = a.astype(np.float64)
    rows = max((a.shape[0] for a in arrays.values() if a.ndim), default=0)
    total = sum(a.size * 8 for a in arrays.values())
    if total > DUMP_LIMIT_BYTES and rows:
        batched = sum(a.size * 8 for a in arrays.values() if a.ndim and a.shape[0] == rows)
        keep = max(1, int(rows * (DUMP_LIMIT_BYTES - (total - batched) - 8 * rows) / batched))
        idx = np.sort(np.random.default_rng(0).choice(rows, size=min(keep, rows), replace=False))
        arrays = {k: a[idx] if a.ndim and a.shape[0] == rows else a for k, a in arrays.items()}
        arrays["rows"] = idx.astype(np.float64)
    os.makedirs(dirname, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(dirname, name + ".npy"), a)


def _flush_c_stdio():
    import ctypes
    try:
        ctypes.CDLL(None).fflush(None)
    except Exception:
        pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--config", choices=("auto", "c3", "c4"), default="auto",
                    help="c3 = configs[2] (1024 spectra per GPU, weak), c4 = configs[3] (one 10 000-spectrum map sharded "
                         "over the ranks, strong); auto = `value` is the c4 map (K steps = K maps, transfers and gather inside) "
                         "on every N, with --full the c3 legs (resident / streamed / one plan for the roofline) beside it on min(K, 8) steps")
    ap.add_argument("--no-scale-reference", action="store_true", help="c3: skip the configs[3] map leg")
    ap.add_argument("--scale-steps", type=int, default=2, help="maps timed by the `scale_reference` leg (one warm-up map before)")
    ap.add_argument("--force-dist", action="store_true",
                    help="create the process group and run every collective through the backend even with ONE rank (a world-1 "
                         "nccl group exercises RCCL, the device binding and the staging on a one-GPU box)")
    ap.add_argument("--batch", type=int, default=1024, help="c3: spectra per GPU per step")
    ap.add_argument("--total", type=int, default=10000, help="c4: spectra of the whole map")
    ap.add_argument("--backend", default=None, help="collectives: rccl (default: RCCL behind the C ABI, no torch), nccl / gloo = "
                                                    "torch.distributed's backends; 'gloo' lets several "
                                                    "ranks share one GPU for a functional check of the N > 1 path")
    ap.add_argument("--shard", choices=("block", "interleave", "lpt"), default="interleave", help="c4: shard scheme")
    ap.add_argument("--inflight", type=lambda v: v if v == "auto" else int(v), default=None,
                    help="batches kept in flight per GPU (each on its own plan + HIP stream); c3 (default 4): steps are dealt "
                         "round-robin to them; c4 (default auto = mapping.auto_inflight(share) = 1: one plan, which cuts the "
                         "share into ranges inside the library): every rank's share is split over them")
    ap.add_argument("--cpu-procs", type=int, default=0, help="worker processes of the all-cores CPU leg (0 = all cpus)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-matrix-build", action="store_true")
    ap.add_argument("--no-other-configs", action="store_true", help="skip the single-spectrum and config-5 timings")
    ap.add_argument("--no-single-caller", action="store_true",
                    help="skip the sub-batched one-caller leg (its launches are half-size: a rocprofv3 --stats average over a run "
                         "with it is not the one-range launch's)")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline, every other leg: c3 legs, rooflines, other configs, matrix build, CPU baselines")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the headline's last timed step returned as DIR/<name>.npy (float64, at most 64 MB)")
    args = ap.parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # launched without torch.distributed.run: this process -- which has not touched the GPU and never will -- starts
        # one fresh child per rank (no exec of a GPU-initialised process), relays rank 0's JSON line and fails if any did
        raise SystemExit(self_launch(args.gpus))
    world_env = int(os.environ.get("WORLD_SIZE", "1"))
    config = args.config if args.config != "auto" else "c3"
    promote = args.config == "auto"          # the c4 map leg of the c3 flow is the headline: K maps timed, `value` = its rate
    c3_steps = min(args.steps, 8) if promote else args.steps

    lib = os.path.join(ROOT, "hybrid-drt_amd", "libhipdrt.so")
    if not os.path.exists(lib) and "HIPDRT_LIB" not in os.environ:      # fresh checkout: build the (git-ignored) library once
        if int(os.environ.get("LOCAL_RANK", "0")) == 0:
            import __graft_entry__
            __graft_entry__.build()                  # the Makefile moves the finished file into place atomically
        else:
            for _ in range(1200):
                if os.path.exists(lib):
                    break
                time.sleep(0.5)
            else:
                raise SystemExit("bench.py: libhipdrt.so did not appear (did rank 0's build fail?)")

    from hipdrt import synth
    cfg = synth.config_c2()
    freq, tau = cfg["freq"], cfg["tau"]
    rank_env = int(os.environ.get("RANK", "0"))

    # ---- CPU legs first: the process pool forks, so it must run before anything in this process has opened the GPU ----
    cpu = None
    if args.full and rank_env == 0 and world_env == 1 and not args.no_cpu_baseline:
        cpu = cpu_baseline(freq, tau, synth.zarc2_batch(freq, 64, first_seed=0), procs=args.cpu_procs)

    import threading
    from hipdrt import _ffi
    from hipdrt.mapping import dist as hd
    from hipdrt.mapping.drtmd import shard_indices
    from hipdrt.models import DRT

    # (no torch in this process unless --backend nccl / gloo asks for torch.distributed: device memory, streams, events and the
    # collectives all sit behind the C ABI -- include/hipdrt.h)
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.backend == "gloo":
        ndev = next((i for i in range(64) if not _ffi.device_usable(i)), 64)
        local %= max(ndev, 1)                            # functional check: ranks may share a GPU
    if not _ffi.device_usable(local):
        raise SystemExit("bench.py needs an MI355X (no CPU fallback)")

    def device_sync():                                   # hipDeviceSynchronize: what torch.cuda.synchronize() is
        plans[0].ctx.device_synchronize()                # (any context of the device will do; no context of its own: no extra stream)
    try:
        # before any fit has touched the GPU: a backend that does not come up ends the run here, non-zero, nothing is restarted
        rank, world, _ = hd.init_from_env(backend=args.backend, device=local, force=args.force_dist)
    except Exception as e:          # noqa: BLE001
        print(f"bench.py: process group initialisation failed: {e!r}", file=sys.stderr)
        raise SystemExit(3)
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    _flush_c_stdio()                                         # (RCCL's start-up banner leaves every rank's buffer now)

    def finish(out, outputs=None, code=0):
        if rank == 0 and args.dump_outputs and outputs is not None:
            dump_outputs(args.dump_outputs, outputs)
        # the JSON line is the LAST thing this job writes to stdout: RCCL prints its banner through C stdio, which is block-buffered
        # on a pipe and would otherwise be flushed at exit, behind the line
        hd.barrier()
        hd.destroy()
        _flush_c_stdio()
        if rank == 0:
            print(json.dumps(out), flush=True)
        if code:
            raise SystemExit(code)

    # ---- BASELINE configs[3] on this N: the headline (`value`) with --config auto, `scale_reference` beside a c3 headline --------
    # (Until round 6 it mattered by 4 % WHERE in the process this ran -- the runtime's placement of the plans' streams on hardware
    # queues, profiles/r06_hw_queue_placement.txt; the library now deals out its own streams by activity and compute pipe,
    # csrc/api.hip: StreamPool, and the order of the legs no longer decides anything.  The map's default is ONE plan, which cuts
    # every rank's share into ranges itself: mapping.auto_inflight.)
    def run_scale_reference():
        scale_ref = got4 = None
        if config == "c3":
            from hipdrt.mapping.drtmd import auto_inflight, fit_observations_sharded
            mine4 = shard_indices(args.total, world, rank, args.shard)
            z4 = np.zeros((args.total, len(freq)), dtype=complex)          # every rank holds its own rows only
            if len(mine4):
                z4[mine4] = np.concatenate([synth.zarc2_batch(freq, 1, first_seed=int(i)) for i in mine4])
            nfl4 = auto_inflight(len(mine4)) if args.inflight in (None, "auto") else args.inflight
            d4 = DRT(fixed_basis_tau=tau, device=local, context=_ffi.Context(local))
            run4 = lambda: fit_observations_sharded(d4, freq, z4, rank=rank, world=world, scheme=args.shard, inflight=nfl4)  # noqa: E731
            maps4 = args.steps if promote else args.scale_steps
            for _ in range(max(1, args.warmup) if promote else 1):
                run4()                                                      # builds the sibling plans; warm-up map(s)
            hd.barrier()
            d4._context.device_synchronize()
            t0 = time.perf_counter()
            for _ in range(maps4):
                got4 = run4()            # upload, fit, llh / rss, download on every rank + ONE gather: returns when rank 0 holds the map
            d4._context.device_synchronize()
            hd.barrier()
            el4 = hd.max_over_ranks(time.perf_counter() - t0)
            if rank == 0:
                # (a reference leg must not take the headline line down: what is wrong with the map is reported in its place)
                ok4 = got4[0].shape == (args.total, len(tau)) and bool(np.isfinite(got4[0]).all()) and bool(got4[2]["obs_fit_status"].all())
                scale_ref = {"value": args.total * maps4 / el4, "unit": "fits/s", "scaling": "strong",
                             "seconds_per_map": el4 / maps4, "maps_timed": maps4, "n_gpus": world,
                             "spectra_per_rank": [len(shard_indices(args.total, world, r, args.shard)) for r in range(world)],
                             "batches_in_flight_per_gpu": nfl4,
                             "workload": (f"BASELINE configs[3]: one map of {args.total} synthetic 2-ZARC spectra (256 x 512) sharded "
                                          f"over {world} rank(s) ({args.shard} shards) by mapping.fit_observations_sharded: per map "
                                          f"upload + full QPHB loop + llh / rss + download on every rank and one gather on rank 0, all "
                                          f"timed (inputs start in HOST memory)")}
                if not ok4:
                    scale_ref["error"] = "the gathered map is incomplete (shape, non-finite coefficients or a failed fit)"
            # plans and contexts go NOW (not whenever the collector gets to them): their memory is free for the legs below
            import gc
            for d_ in [d4] + list(getattr(d4, "_sibling_clones", None) or []):
                if getattr(d_, "_plan", None) is not None:
                    d_._plan.close()
                    d_._plan = d_._plan_key = None
                if d_._context is not None:
                    d_._context.close()
            del d4, z4
            gc.collect()
        return scale_ref, got4

    if promote and not args.full:
        # a plain run: the headline alone -- the configs[3] map, K maps timed; its result is also what --dump-outputs writes
        scale_ref, got4 = run_scale_reference()
        out = None
        if rank == 0:
            out = {"metric": "DRT fits/sec (256 freq x 512 tau, batched)", "value": scale_ref["value"], "unit": "fits/s",
                   "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                   "ms_per_step": scale_ref["seconds_per_map"] * 1e3, "higher_is_better": True, "scaling": "strong",
                   "vs_baseline": None, "dtype": "f64", "data": "synthetic",
                   "config": {"workload": scale_ref["workload"] + f" -- a step = one whole map; TRANSFERS ARE INSIDE: the {args.total} "
                                          f"x 256 complex spectra start in host memory, the results ({len(tau) + 9} doubles per "
                                          f"spectrum) are downloaded and gathered on rank 0 in every step",
                              "nf": len(freq), "ntau": len(tau), "spectra_per_map": args.total,
                              "spectra_per_rank": scale_ref["spectra_per_rank"],
                              "batches_in_flight_per_gpu": scale_ref["batches_in_flight_per_gpu"]},
                   "scale_reference": scale_ref,
                   "collectives": {"backend": hd.backend(), "forced_one_rank_group": bool(hd.forced()),
                                   "torch_imported": "torch" in sys.modules},
                   "full": False}
        # (an incomplete map is the headline's own failure here: the line says so and the run exits non-zero)
        bad = rank == 0 and "error" in scale_ref
        finish(out, map_outputs(got4) if rank == 0 else None, code=1 if bad else 0)
        return

    if config == "c3":
        B = args.batch
        z = synth.zarc2_batch(freq, B, first_seed=rank * B)
        nfl = max(1, min(4 if args.inflight in (None, "auto") else args.inflight, max(c3_steps, 1)))
        chunks = [np.arange(B)] * nfl                        # every plan holds the whole batch
        job_fits = world * B
    else:
        total = args.total
        mine = shard_indices(total, world, rank, args.shard)
        z_all = None
        # every rank generates its own rows only (seed = global observation index)
        z = np.concatenate([synth.zarc2_batch(freq, 1, first_seed=int(i)) for i in mine]) if len(mine) else \
            np.zeros((0, len(freq)), dtype=complex)
        from hipdrt.mapping.drtmd import auto_inflight
        nfl = auto_inflight(len(mine)) if args.inflight in (None, "auto") else args.inflight
        nfl = max(1, min(nfl, max(len(mine), 1)))
        chunks = np.array_split(np.arange(len(mine)), nfl)
        B = len(mine)
        job_fits = total

    scale_ref = got4 = None

    # one DRT + plan + HIP stream per in-flight batch
    if config == "c3":
        drts = [DRT(fixed_basis_tau=tau, device=local, context=_ffi.Context(local)) for _ in range(nfl)]
        plans = [d.stage_batch(freq, z[c]) for d, c in zip(drts, chunks)]     # lookups + matrices built, spectra resident
        for p_ in plans:
            p_.set_subbatches(1)          # the legs below choose: several plans of ONE launch sequence each, or one plan that cuts its batch itself
    else:
        # c4 goes through the product's own driver (mapping.fit_observations_sharded: shard -> `nfl` batches side by side
        # on sibling plans -> one gather); this first call builds the sibling plans
        from hipdrt.mapping.drtmd import drt_siblings, fit_observations_sharded
        z_all = np.zeros((total, len(freq)), dtype=complex)
        z_all[mine] = z                                   # every rank holds its own rows only
        drt0 = DRT(fixed_basis_tau=tau, device=local, context=_ffi.Context(local))
        fit_observations_sharded(drt0, freq, z_all, rank=rank, world=world, scheme=args.shard, inflight=nfl)
        drts = drt_siblings(drt0, nfl) if len(mine) >= 2 * nfl else [drt0]
        nfl = len(drts)
        plans = [d._plan for d in drts]
    drt, plan = drts[0], plans[0]
    if plan is None:
        raise SystemExit(f"bench.py: rank {rank} has no observations to fit ({job_fits} spectra over {world} ranks)")
    if hd.active(world) and config == "c3":
        # rank 0's lookup tables -> everyone, one RCCL broadcast (c4: mapping.fit_observations_sharded does this itself)
        from hipdrt.mapping.drtmd import share_lookup_tables
        for d in drts:
            share_lookup_tables(d, rank, world, src=0)

    for d in drts:
        for _ in range(args.warmup if config == "c3" else 0):
            d.fit_staged()
    for _ in range(args.warmup if config == "c4" else 0):
        fit_observations_sharded(drt, freq, z_all, rank=rank, world=world, scheme=args.shard, inflight=nfl)

    stats = [dict(qp_ms=0.0, qp_launch=0, phase={"gram": 0.0, "qp": 0.0, "hyper": 0.0}) for _ in range(nfl)]
    results = [None] * nfl

    def note(i):
        tms, launches = plans[i].timings()
        stats[i]["qp_ms"] += tms["qp"]
        stats[i]["qp_launch"] += launches["qp"]
        for k in stats[i]["phase"]:
            stats[i]["phase"][k] += tms[k]

    def worker_resident(i, nsteps):                       # c3: inputs resident, results stay on the device
        for _ in range(nsteps):
            drts[i].fit_staged()                          # returns after the plan's stream has drained
            note(i)

    def worker_transfers(i, nsteps):                      # upload + fit + download per step (c4; c3's second leg)
        for _ in range(nsteps):
            plans[i].upload(z[chunks[i]])
            drts[i].fit_staged()
            results[i] = drts[i].collect_staged()
            note(i)

    def sync_all():
        device_sync()
        for p_ in plans:
            p_.ctx.synchronize()

    def timed_c3(nfl_used, worker):
        share = [c3_steps // nfl_used + (1 if i < c3_steps % nfl_used else 0) for i in range(nfl_used)]
        hd.barrier()
        sync_all()
        t0 = time.perf_counter()
        threads = [threading.Thread(target=worker, args=(i, share[i])) for i in range(nfl_used)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        sync_all()
        hd.barrier()
        return hd.max_over_ranks(time.perf_counter() - t0)

    counts = [len(shard_indices(args.total, world, r, args.shard)) for r in range(world)] if config == "c4" else None

    def timed_c4():
        hd.barrier()
        sync_all()
        t0 = time.perf_counter()
        gathered = None
        for _ in range(args.steps):
            # upload, fit, llh / rss, download on every rank and ONE gather, all inside the product's driver
            gathered = fit_observations_sharded(drt, freq, z_all, rank=rank, world=world, scheme=args.shard, inflight=nfl)
            for i in range(nfl):
                note(i)
        sync_all()
        hd.barrier()
        return hd.max_over_ranks(time.perf_counter() - t0), gathered

    reset = lambda: [s_.update(qp_ms=0.0, qp_launch=0, phase={"gram": 0.0, "qp": 0.0, "hyper": 0.0}) for s_ in stats]  # noqa: E731
    single_elapsed = transfer_elapsed = one_caller_elapsed = None
    if config == "c3":
        elapsed = timed_c3(nfl, worker_resident)
        if args.full:
            reset()
            transfer_elapsed = timed_c3(nfl, worker_transfers)      # same steps with upload and download inside
            reset()
            single_elapsed = timed_c3(1, worker_resident)           # one batch in flight: un-overlapped launches
        qp_ms, qp_launch = stats[0]["qp_ms"], stats[0]["qp_launch"]
        phase = dict(stats[0]["phase"])
        # the configs[3] map: behind the four configs[2] plans' streams (queues 0..3: its three land on 4, 5, 6) and in front of
        # the one-caller leg, whose ranges make two more streams
        if args.full and not args.no_scale_reference:
            scale_ref, got4 = run_scale_reference()
        if args.full and not args.no_single_caller:
            plans[0].set_subbatches(0)                              # one caller, one plan, the library cuts the batch into ranges
            one_caller_elapsed = timed_c3(1, worker_resident)
            plans[0].set_subbatches(1)
        steps_in_stats = c3_steps
        res = drt.collect_staged()
    else:
        elapsed, gathered = timed_c4()
        qp_ms = sum(s_["qp_ms"] for s_ in stats)
        qp_launch = sum(s_["qp_launch"] for s_ in stats)
        phase = {k: sum(s_["phase"][k] for s_ in stats) for k in ("gram", "qp", "hyper")}
        steps_in_stats = args.steps
        res = None
        if rank == 0:
            obs_x, obs_special, res_all = gathered
            assert obs_x.shape == (args.total, len(tau)) and np.isfinite(obs_x).all() and res_all["obs_fit_status"].all()
            res = {k: res_all[k][mine] for k in ("outer_iters", "qp_iters_total", "status")}     # this rank's share

    n, m = plan.n, plan.m
    out = None
    if rank == 0:
        n_qp = res["outer_iters"].astype(np.int64) + 1
        flop_batch = float(qp_algorithmic_flop(n, res["qp_iters_total"].astype(np.int64), n_qp).sum())   # one plan's batch
        # c3: `res` is one plan's batch; c4: this rank's whole share, whose launches are spread over its plans
        launches_batch = qp_launch / max(steps_in_stats, 1)
        flop_per_launch = flop_batch / launches_batch
        avg_launch_s = qp_ms / max(qp_launch, 1) / 1e3
        achieved = flop_per_launch / avg_launch_s / 1e12
        traffic, traffic_note = None, "no PMC figure committed"
        pmc = os.path.join(ROOT, "profiles", "qp_traffic.json")
        if os.path.exists(pmc) and config == "c3":
            try:
                rec = json.load(open(pmc))
                if rec.get("source_hash") == source_hash() and rec.get("kernel") == QP_KERNEL:
                    traffic, traffic_note = rec.get("hbm_bytes_per_launch"), "rocprofv3 --pmc passes on these sources (profiles/qp_traffic.json)"
                else:
                    traffic_note = "profiles/qp_traffic.json was measured on other sources or another kernel: not reported"
            except Exception:
                traffic_note = "profiles/qp_traffic.json unreadable"
        alg_bytes_fact = (n * n + n * (n + 1) / 2.0) * 8.0
        fact_per_launch = float((res["qp_iters_total"].astype(np.int64) + n_qp).sum()) / launches_batch
        value = job_fits * (c3_steps if config == "c3" else args.steps) / elapsed
        nb = len(res["outer_iters"])
        outer_sum = float(res["outer_iters"].sum())
        # (c4: `res` is the rank's whole share, so the times are summed over its plans as if they ran one after the other)
        gram_s = phase["gram"] / steps_in_stats / 1e3
        hyper_s = phase["hyper"] / steps_in_stats / 1e3
        gram_flop = (outer_sum + nb) * m * n * n            # lower triangle of A'WA: m n^2 per spectrum and QP
        out = {
            "metric": "DRT fits/sec (256 freq x 512 tau, batched)", "value": value, "unit": "fits/s",
            # the two forms of the headline side by side (bench contract: `value` = inputs resident in HBM when the timed region
            # starts; SURVEY 8d's "B / wall including H2D / D2H" is `value_streamed`: the same K steps with the upload of the
            # spectra and the download of every result inside each step)
            "value_streamed": None if transfer_elapsed is None else world * B * c3_steps / transfer_elapsed,
            "value_resident": value,
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": elapsed / (c3_steps if config == "c3" else args.steps) * 1e3, "higher_is_better": True,
            "scaling": "weak" if config == "c3" else "strong",
            "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": (f"BASELINE configs[2]: {B} synthetic 2-ZARC spectra per GPU, shared 256-point frequency "
                                    f"grid x 512-point tau grid, full QPHB loop (DRT.fit_eis defaults, interp lookups), "
                                    f"inputs resident in HBM (`value`, `value_resident`); `value_streamed` = the same steps with "
                                    f"upload + download inside; weak scaling: every rank fits its own {B} spectra, no data-path "
                                    f"collective; the configs[3] map on the same N is `scale_reference`") if config == "c3" else
                                   (f"BASELINE configs[3]: one map of {args.total} synthetic 2-ZARC spectra (256 x 512) "
                                    f"sharded over {world} rank(s) ({args.shard} shards) by mapping.fit_observations_sharded: "
                                    f"per step upload + full QPHB loop + llh / rss + download on every rank and one "
                                    f"gather on rank 0"),
                       "batch_per_gpu": B, "nf": 256, "ntau": 512, "n_unknowns": n,
                       "sharding": (f"{world} rank(s) x {B} independent spectra, no data-path collective" if config == "c3"
                                    else f"{args.total} spectra over {world} rank(s), {counts} per rank, one gather to rank 0 "
                                         f"of {len(tau) + 9} doubles per spectrum per map (lookup tables broadcast once, "
                                         f"before the timed region)"),
                       "batches_in_flight_per_gpu": nfl,
                       "converged_fraction": float((res["status"] == 0).mean()),
                       "mean_outer_iterations": float(res["outer_iters"].mean()),
                       "mean_ipm_iterations_per_fit": float(res["qp_iters_total"].mean())},
            "roofline": {"bound": "mfma", "kernel": QP_KERNEL,
                         "achieved": achieved, "peak": FP64_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                         "frac": achieved / FP64_MFMA_PEAK_TFLOPS, "traffic": traffic, "traffic_note": traffic_note,
                         "flop_per_launch": flop_per_launch, "avg_launch_ms": avg_launch_s * 1e3,
                         "launches_per_step": launches_batch,
                         "measured_on": ("single_stream: HIP-event launch times, phase split and this fraction come from the leg "
                                         "with ONE batch in flight (un-overlapped launches); `value` is the multi-plan leg, in "
                                         "which launches of different plans overlap") if config == "c3" else "c4 plans in flight",
                         "flop_convention": "SURVEY 8d: n^3/3 + 2*2*n^2 per IPM iteration, n^3/3 + 2 n^2 per start point",
                         # the same launch against the other roof: PMC bytes / HIP-event time
                         "traffic_GBps": None if traffic is None else traffic / avg_launch_s / 1e9,
                         "traffic_frac_of_hbm_peak": None if traffic is None else traffic / avg_launch_s / 8e12,
                         "note": None if config == "c3" else
                         "c4: launch times are HIP-event intervals on streams that share the GPU with the other plans in "
                         "flight, i.e. inflated by the overlap; the kernel's roofline figure is the c3 line's"},
            # the same kernel against the other roof: SURVEY 8d's algorithmic bytes of a factorisation are the
            # P read (n^2 doubles) and the factor write (n (n + 1) / 2 doubles); `traffic` is what the PMC counters saw
            "roofline_hbm": {"bound": "hbm", "kernel": QP_KERNEL,
                             "algorithmic_bytes_per_factorisation": alg_bytes_fact,
                             "factorisations_per_launch": fact_per_launch,
                             "algorithmic_bytes_per_launch": alg_bytes_fact * fact_per_launch,
                             "achieved": alg_bytes_fact * fact_per_launch / avg_launch_s / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                             "frac": alg_bytes_fact * fact_per_launch / avg_launch_s / 1e9 / HBM_PEAK_GBS,
                             "traffic": traffic, "traffic_note": traffic_note,
                             "traffic_over_algorithmic": None if traffic is None else traffic / (alg_bytes_fact * fact_per_launch),
                             "traffic_bytes_per_factorisation": None if traffic is None else traffic / fact_per_launch,
                             "traffic_GBps": None if traffic is None else traffic / avg_launch_s / 1e9,
                             "traffic_frac_of_hbm_peak": None if traffic is None else traffic / avg_launch_s / 1e9 / HBM_PEAK_GBS,
                             "avg_launch_ms": avg_launch_s * 1e3},
            "roofline_gram": {"bound": "mfma", "kernel": "gram_kernel", "ms_per_step": gram_s * 1e3,
                              "achieved": gram_flop / max(gram_s, 1e-12) / 1e12, "peak": FP64_MFMA_PEAK_TFLOPS,
                              "unit": "TFLOP/s", "frac": gram_flop / max(gram_s, 1e-12) / 1e12 / FP64_MFMA_PEAK_TFLOPS,
                              "note": "m n^2 flop per spectrum and QP (lower triangle only; SURVEY's 2 m n^2 counts the "
                                      "mirrored half as well: double this fraction for that convention)"},
            "roofline_hyper": {"bound": "l2", "kernel": "hyper_kernel", "ms_per_step": hyper_s * 1e3,
                               "achieved": outer_sum * (m * n + m * m) * 8 / max(hyper_s, 1e-12) / 1e9,
                               "unit": "GB/s", "frac": None,
                               "note": "algorithmic bytes = (m n + m^2) 8 per spectrum and outer iteration (the two "
                                       "matrix-vector products of estimate_weights); the matrices are shared by the "
                                       "batch and are served by L2 / Infinity Cache, not HBM: no HBM fraction is quoted"},
            "phase_ms_per_step": {k: v / steps_in_stats / (1 if config == "c3" else nfl) for k, v in phase.items()},
            "single_stream": None if single_elapsed is None else {
                "value": world * B * c3_steps / single_elapsed, "ms_per_step": single_elapsed / c3_steps * 1e3,
                "note": "same K steps with one batch in flight; roofline / phase timings are taken from this run"},
            "single_caller": None if one_caller_elapsed is None else {
                "value": world * B * c3_steps / one_caller_elapsed, "ms_per_step": one_caller_elapsed / c3_steps * 1e3,
                "note": "same K steps from ONE caller thread on ONE plan (one plan's memory): hipdrt_plan_fit cuts the staged batch "
                        "into ranges that run side by side on the plan's own streams (hipdrt_plan_set_subbatches, automatic)"},
            "scale_reference": scale_ref,
            # how the ranks talk: 'rccl' = RCCL behind the C ABI (hipdrt_comm_*), 'nccl' / 'gloo' = torch.distributed; None = one
            # rank, no group.  The native path never imports torch.
            "collectives": {"backend": hd.backend(), "forced_one_rank_group": bool(hd.forced()), "torch_imported": "torch" in sys.modules},
            "with_transfers": None if transfer_elapsed is None else {
                "value": world * B * c3_steps / transfer_elapsed, "ms_per_step": transfer_elapsed / c3_steps * 1e3,
                "note": "same K steps with the upload of the spectra and the download of all results inside every step"},
        }
        if args.full and not args.no_matrix_build:
            # secondary roofline (north_star): batched Z'/Z'' build with per-spectrum frequency grids
            Bm = 512
            fb = np.sort(10 ** np.random.default_rng(0).uniform(-1, 6, size=(Bm, 256)), axis=1)[:, ::-1].copy()
            lk = drt.interpolate_lookups
            dre, dim = plan.ctx.device_alloc(Bm * 256 * 512 * 8), plan.ctx.device_alloc(Bm * 256 * 512 * 8)
            plan.ctx.impedance_matrix_timed(fb, tau, drt.tau_epsilon, dre, dim, lookups=(lk["z_real"], lk["z_imag"]), repeat=1)
            reps = 10
            ms = plan.ctx.impedance_matrix_timed(fb, tau, drt.tau_epsilon, dre, dim, lookups=(lk["z_real"], lk["z_imag"]),
                                                 repeat=reps)
            plan.ctx.device_free(dre)
            plan.ctx.device_free(dim)
            byts = Bm * 2 * 256 * 512 * 8
            gbs = byts * reps / (ms / 1e3) / 1e9
            out["matrix_build_roofline"] = {"bound": "hbm", "kernel": "impedance_interp_kernel",
                                            "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                            "frac": gbs / HBM_PEAK_GBS, "bytes_per_launch": byts,
                                            "avg_launch_ms": ms / reps}
        if args.full and world == 1 and not args.no_other_configs:
            # the other BASELINE configs as measured here (parity cases, not the bench metric): configs[1] one spectrum
            # 256 x 512, configs[4] one joint chrono + EIS fit with DOP (512 f + 4096 t x 1024 tau); wall time of the
            # second call (plans and lookup tables warm), inputs handed over as host arrays
            other = {}
            z1 = synth.zarc2_batch(freq, 1, first_seed=0)
            drt.fit_eis_batch(freq, z1)
            t0 = time.perf_counter()
            one = drt.fit_eis_batch(freq, z1)
            t_gpu1 = time.perf_counter() - t0
            other["config1_single_spectrum_256x512"] = {"seconds": t_gpu1, "outer_iterations": int(one["outer_iters"][0])}
            meas = synth.hybrid_measurement(seed=0, n_pre=96, n_post=4000, nf=512)
            d5 = DRT(fixed_basis_tau=np.logspace(-7, 3, 1024), fit_dop=True, warn=False, device=local)
            d5.fit_hybrid(*meas, max_iter=2)
            t0 = time.perf_counter()
            d5.fit_hybrid(*meas)
            tm5 = d5._plan.timings()[0]
            t_gpu5 = time.perf_counter() - t0
            it5 = int(d5.qphb_params["outer_iterations"])
            other["config4_joint_fit_dop_512f_4096t_1024tau"] = {
                "seconds": t_gpu5, "device_loop_seconds": tm5["total"] / 1e3,
                "qp_seconds": tm5["qp"] / 1e3, "rows": int(d5.qphb_params["rm"].shape[0]),
                "unknowns": int(d5.qphb_params["rm"].shape[1]), "outer_iterations": it5,
                "note": "2 uV of voltage noise: the reference's own outer loop is not contractive on this workload -- the answer is "
                        "not reproducible beyond outer iteration 6 in any implementation (tests/golden/refrun_config5_2uV pins those "
                        "six); the timing is of the full 50 iterations.  The call before it fitted the same protocol on the same object: "
                        "the penalty / variance / impedance blocks are kept from it, as upstream keeps its fit matrices while the "
                        "sampling does not change -- the first fit of a protocol takes about 0.08 s longer"}
            # the same fit on the CONTRACTIVE workload (20 uV of voltage noise; tests/golden/refrun_config5_full pins its first
            # twelve outer iterations against the reference's own run at 4.8e-10 of the peak)
            meas20 = synth.hybrid_measurement(seed=0, n_pre=96, n_post=4000, nf=512, v_noise=2e-5)
            d5.fit_hybrid(*meas20, max_iter=2)
            t0 = time.perf_counter()
            d5.fit_hybrid(*meas20)
            t_gpu20 = time.perf_counter() - t0
            tm20 = d5._plan.timings()[0]
            other["config4_joint_fit_dop_20uV_contractive"] = {
                "seconds": t_gpu20, "device_loop_seconds": tm20["total"] / 1e3, "qp_seconds": tm20["qp"] / 1e3,
                "outer_iterations": int(d5.qphb_params["outer_iterations"])}
            if not args.no_cpu_baseline:
                # 1-core CPU legs of these two configs: the oracle in this process (single-threaded BLAS, see the top of the
                # file; nothing is forked here).  configs[1]: the same spectrum, the whole fit.  configs[4]: the oracle's loop
                # on the device-built matrices for the first K outer iterations (a full fit takes minutes on one core); the
                # GPU figure beside it is the device loop's time for the same K iterations.
                from oracle import drt_oracle as orc
                odrt = orc.OracleDRT(fixed_basis_tau=tau)
                odrt.prepare(freq)
                t0 = time.perf_counter()
                odrt.fit_eis(freq, z1[0], structure='fast')
                t_cpu1 = time.perf_counter() - t0
                other["config1_single_spectrum_256x512"]["cpu_baseline"] = {
                    "value": t_cpu1, "unit": "s per fit", "cores": 1, "kind": "port",
                    "sample": "the same spectrum, whole fit, oracle/drt_oracle.py structure='fast', 1 BLAS thread",
                    "gpu_over_cpu_core": t_cpu1 / t_gpu1}
                K5 = 2
                d5.fit_hybrid(*meas, max_iter=K5)
                gpu_k = d5._plan.timings()[0]["total"] / 1e3
                qp5, special5 = d5.qphb_params, d5.special_qp_params
                rzm0 = qp5["rm"].copy()
                vi = special5["vz_offset"]["index"]
                rzm0[:, vi] = 0
                vb = special5["v_baseline"]
                vz = dict(index=vi, strength=qp5["vz_strength_vec"], num_chrono=qp5["num_chrono"],
                          vb=(vb["index"], vb["index"] + vb["size"]))
                hyp = orc.get_default_hypers()
                hyp.update(orc.get_default_dop_hypers())
                t0 = time.perf_counter()
                orc.qphb_fit_prepared(rzm0, qp5["rv"], [qp5["penalty_matrices"][f"m{k}"] for k in range(3)], qp5["vmm"],
                                      special5, hyp, vz=vz, max_iter=K5, keep_history=False)
                t_cpu5 = time.perf_counter() - t0
                other["config4_joint_fit_dop_512f_4096t_1024tau"]["cpu_baseline"] = {
                    "value": t_cpu5, "unit": f"s per {K5} outer iterations (+ the initial-weights QP)", "cores": 1, "kind": "port",
                    "sample": f"oracle.qphb_fit_prepared on the device-built matrices (5120 x 1078), max_iter={K5}, 1 BLAS thread; "
                              f"the device loop took {gpu_k:.3f} s for the same {K5} iterations",
                    "gpu_seconds_same_sample": gpu_k, "gpu_over_cpu_core": t_cpu5 / max(gpu_k, 1e-9)}
            out["other_configs"] = other
        if promote and scale_ref is not None and "error" not in scale_ref:
            # `value` = BASELINE configs[3] (the workload the metric is quoted on at 1 / 2 / 4 / 8 GPUs): K whole maps, everything a
            # caller of mapping.fit_observations_sharded waits for inside the timed region.  The c3 figures stay in the line.
            out["c3"] = {"value": value, "ms_per_step": out["ms_per_step"], "steps": c3_steps, "scaling": "weak",
                         "workload": out["config"]["workload"].replace("(`value`, `value_resident`)", "(`value_resident`)")
                         .replace("the configs[3] map on the same N is `scale_reference`",
                                  "the configs[3] map on the same N is this line's `value` (and `scale_reference`)")}
            value = scale_ref["value"]
            out["value"] = value
            out["ms_per_step"] = scale_ref["seconds_per_map"] * 1e3
            out["scaling"] = "strong"
            out["config"]["workload"] = (
                scale_ref["workload"] + f" -- a step = one whole map; TRANSFERS ARE INSIDE: the {args.total} x 256 complex spectra start "
                f"in host memory (upload {args.total * 256 * 16 / 1e6:.0f} MB per map), the results ({len(tau) + 9} doubles per spectrum) "
                f"are downloaded and gathered on rank 0 in every step (SURVEY 8d: fits/s = B / wall including H2D / D2H).  "
                f"`value_resident` / `value_streamed` are BASELINE configs[2] ({B} spectra per GPU, weak scaling, {c3_steps} steps) with "
                f"inputs resident in HBM / with upload + download inside; `roofline` is measured on its one-plan leg (`single_stream`)")
            out["config"]["spectra_per_map"] = args.total
            out["config"]["spectra_per_rank"] = scale_ref["spectra_per_rank"]
            out["config"]["sharding"] = (f"{args.total} spectra over {world} rank(s) ({args.shard} shards), no data-path collective during "
                                         f"the fit, one gather to rank 0 per map (lookup tables broadcast once, before the timed region)")
            out["config"]["batches_in_flight_per_gpu"] = scale_ref["batches_in_flight_per_gpu"]
        if cpu is not None:
            out["cpu_baseline"] = cpu
            cpu["gpu_over_cpu_core"] = value / cpu["value"]
            if cpu["all_cores"] and cpu["all_cores"]["value"]:
                cpu["gpu_over_all_cores"] = value / cpu["all_cores"]["value"]
            cpu["gpu_over_reference_structure"] = value / cpu["reference_structure"]["value"]
        else:
            out["cpu_baseline"] = None
        out["full"] = args.full
        if not args.full:                                   # a plain c3 / c4 run: its first leg's headline alone
            out = {k: out[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                                       "scaling", "vs_baseline", "dtype", "data", "config", "collectives", "full")}
    outputs = None
    if rank == 0:
        if promote and scale_ref is not None and "error" not in scale_ref:
            outputs = map_outputs(got4)                     # the headline is the map
        elif config == "c3":
            outputs = res                                   # one plan's batch (every plan fits the same spectra)
        else:
            outputs = map_outputs(gathered)
    finish(out, outputs)


if __name__ == "__main__":
    main()
