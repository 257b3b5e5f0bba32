#!/usr/bin/env python3
"""bench.py -- Mbursts/s detect+demod (156.25 symbols, 4 SPS) on N MI355X GPUs of one node.

A "step" is one pass of the hot path (trxhip_detect_demod_batch: int16 IQ -> energy/RSSI -> detect ->
demod -> soft bits) over one device-resident batch of synthetic bursts: BASELINE.json configs[1],
1M normal bursts per GPU, 4 SPS, all 8 TSCs.  N > 1 = weak scaling: every rank processes its own
1M-burst shard; the only collective is the init-time RCCL broadcast of the table blob.

  python bench.py --gpus N --steps K --warmup W          (driver launches N>1 under torch.distributed.run)

Prints ONE JSON line on rank 0 (see DESIGN.md "Measurement" for every field); `ms_per_step` is the wall time of one
of the K timed steps.  `--dump-outputs DIR` also writes what the last timed step computed (a fixed, seeded sample of
bursts) as DIR/<name>.npy; the inputs are seeded, so two builds run with the same arguments compare output for output.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import re
FUSED_SOFT_ATOL = float(re.search(r"#define\s+TRXHIP_FUSED_SOFT_ATOL\s+([0-9.eE+-]+)f?\b",       # the one tolerance statement
                                  open(os.path.join(ROOT, "include", "trxhip.h")).read()).group(1))
FAST_AMP_RTOL = float(re.search(r"#define\s+TRXHIP_FAST_AMP_RTOL\s+([0-9.eE+-]+)f?\b",
                                open(os.path.join(ROOT, "include", "trxhip.h")).read()).group(1))
BYTES_PER_BURST = 3132          # 2500 B int16 IQ + 8 B params + 592 B soft bits + 32 B result
HBM_PEAK_GBS = 8000.0           # MI355X_MICROARCH.md: HBM3E 8 TB/s spec


def usable_cores():
    """Host threads this process can actually run: the affinity mask, capped by the cgroup CPU quota."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = max(1, min(n, int(-(-int(quota) // int(period)))))
    except Exception:
        pass
    return n


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except Exception:
        pass
    return "unknown"


def cpu_baseline(iq_host, params, target_seconds=6.0):
    """Time the CPU oracle (oracle/trx_oracle.c, a port of the reference's generic-C path, gcc -O2) on a
    bounded sample of the same workload: one thread per usable host core, each thread looping over its own
    contiguous slice of the sample (bursts are independent, so a static split is the fair CPU ceiling;
    ctypes releases the GIL).  A one-pass calibration sizes the repeat count to ~target_seconds.

    Second entry (`sse_path`), when oracle/_ref/libref_sse.so travelled with the snapshot: the same call graph with every
    FIR executed by the reference's OWN SSE3 kernels (arch/x86/convolve_sse_3.c compiled unmodified; orc_set_arch) and the
    reference's per-call padded copies -- the reference's x86 path as closely as this image can build it (sigProcLib.cpp
    itself needs libosmocore headers the image lacks)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib as O
    from concurrent.futures import ThreadPoolExecutor
    cores = usable_cores()
    O.lib()
    n_sample = len(iq_host)
    per = max(256, n_sample // cores)
    slices = [(min(i * per, n_sample - per), min(i * per, n_sample - per) + per) for i in range(cores)]

    def timed(seconds):
        n1 = min(n_sample, 8192)
        t0 = time.perf_counter()
        O.pull_batch(iq_host[:n1], 4, params[:n1])
        t1 = time.perf_counter() - t0

        def run(reps):
            def work(b):
                for _ in range(reps):
                    O.pull_batch(iq_host[b[0]:b[1]], 4, params[b[0]:b[1]])
            t0 = time.perf_counter()
            with ThreadPoolExecutor(cores) as ex:
                list(ex.map(work, slices))
            return time.perf_counter() - t0

        tcal = run(1)                                                # calibration pass, all threads
        reps = max(1, min(200, int(seconds / max(tcal, 1e-3))))
        tn = run(reps)
        return per * reps * cores, tn, reps, n1 / t1

    done, tn, reps, single = timed(target_seconds)
    out = {
        "value": round(done / tn / 1e6, 6), "unit": "Mbursts/s", "cores": cores, "kind": "port",
        "sample": f"first {n_sample} bursts of the same batch split over {cores} threads ({per} bursts each, "
                  f"repeated {reps}x: {done} bursts in {tn:.1f} s); oracle/trx_oracle.c, generic-C order, gcc -O2",
        "single_thread_kbursts_s": round(single / 1e3, 2),
        "cpu_model": cpu_model(),
        "host": {"affinity_cpus": len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else None,
                 "cgroup_cpu_max": (open("/sys/fs/cgroup/cpu.max").read().strip()
                                    if os.path.exists("/sys/fs/cgroup/cpu.max") else None)},
    }
    if O.ref_arch_available("sse"):
        try:
            O.use_ref_arch("sse")
            done2, tn2, reps2, single2 = timed(target_seconds * 0.6)
            out["sse_path"] = {
                "value": round(done2 / tn2 / 1e6, 6), "unit": "Mbursts/s", "cores": cores, "kind": "port",
                "kernels": "the reference's own arch/x86 SSE3 convolve kernels, compiled unmodified (oracle/_ref/libref_sse.so), at "
                           "every convolve() call site incl. the reference's per-call padded copy and aligned taps",
                "sample": f"same sample and split, repeated {reps2}x: {done2} bursts in {tn2:.1f} s",
                "single_thread_kbursts_s": round(single2 / 1e3, 2)}
        finally:
            O.use_ref_arch(None)
    return out


def side_legs(args, trx, synth, shard, step, iq, n, dev, rank, world, results, soft):
    """Side measurements reported inside `config` (never `value`): exact demodulator, configs[4] mix, host-fed path."""
    import numpy as np
    import torch
    # the bit-exact two-stage demodulator on the same batch
    xs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(5)]
    warm_clocks(lambda: step(exact=True))
    for a, b in xs:
        a.record()
        step(exact=True)
        b.record()
    torch.cuda.synchronize()
    exact_ms = sum(a.elapsed_time(b) for a, b in xs) / len(xs)

    # side measurement (not `value`): BASELINE.json configs[4]'s per-GPU share, the 7:1 NB:RACH mix (RACH max_toa 63)
    iq_m, params_m = synth.make_mixed_bursts(n, dev, seed=synth.SEED + 2 + 1000003 * rank)
    d_params_m = trx.params_tensor(params_m)

    from osmo_trx_amd import trxhip
    hint_m = trxhip.few_nb_hint(params_m)                           # (once: a pass over the host copy of the slot table)

    def step_mixed():
        trx.detect_demod(iq_m, d_params_m, sps=4, soft_stride=148, slice_bits=True, results=results, soft=soft, hint=hint_m)

    warm_clocks(step_mixed)
    shard.barrier()
    t0m = time.perf_counter()
    for _ in range(5):
        step_mixed()
    torch.cuda.synchronize()
    shard.barrier()
    mixed_s = shard.max_over_ranks(time.perf_counter() - t0m, dev if shard.backend_name() else None)
    mixed_detected = int((trx.results_to_numpy(results)["rc"] > 0).sum())

    # side measurement (not `value`): host-fed, PCIe-inclusive.  Bursts sit in pinned host memory (where a producer such
    # as BurstGatherer writes them), every slot runs H2D -> detect/demod -> TRXD pack -> D2H on its own stream.
    host_fed = None
    if rank == 0 and not args.no_host_fed:
        from osmo_trx_amd.trxhip import HostPipe, TRXD_META_DTYPE
        hb, depth, iters = 16384, 4, 48
        pipe = HostPipe(trx, hb, depth=depth, soft_stride=0, pkt_stride=160)
        h_iq = np.ascontiguousarray(iq_m[: hb * depth].cpu().numpy())
        for sl in range(depth):
            v = pipe.slot(sl)
            v["iq"][:] = h_iq[sl * hb:(sl + 1) * hb]
            v["params"][:] = params_m[sl * hb:(sl + 1) * hb]
            v["meta"][:] = np.zeros(hb, dtype=TRXD_META_DTYPE)
            v["meta"]["version"] = 1
        for sl in range(depth):
            pipe.submit(sl, hb)
        for sl in range(depth):
            pipe.wait(sl)
        t0h = time.perf_counter()
        for it in range(iters):
            sl = it % depth
            pipe.wait(sl)
            pipe.submit(sl, hb)
        for sl in range(depth):
            pipe.wait(sl)
        th = time.perf_counter() - t0h
        # the same batches BY REFERENCE (round 5): the bursts stay in a registered host range (the radio's receive ring), the slot
        # carries their addresses and a device kernel fetches them over the link -- no CPU copy in front of the pipe at all
        pipe.register_host(h_iq)
        for sl in range(depth):
            pipe.sources(sl)[:] = h_iq.ctypes.data + 2500 * (sl * hb + np.arange(hb, dtype=np.uint64))
            pipe.submit_by_ref(sl, hb)
        for sl in range(depth):
            pipe.wait(sl)
        t0r = time.perf_counter()
        for it in range(iters):
            sl = it % depth
            pipe.wait(sl)
            pipe.submit_by_ref(sl, hb)
        for sl in range(depth):
            pipe.wait(sl)
        tr = time.perf_counter() - t0r
        up, down = hb * (625 * 4 + 8 + 8), hb * (32 + 160 + 2)
        host_fed = {"mbursts_per_s": round(iters * hb / th / 1e6, 3), "h2d_GBps": round(iters * up / th / 1e9, 2),
                    "d2h_GBps": round(iters * down / th / 1e9, 2), "bursts_per_submit": hb, "slots": depth,
                    "by_reference_mbursts_per_s": round(iters * hb / tr / 1e6, 3),
                    "by_reference_note": "trxhip_hostpipe_submit_by_ref: bursts fetched by a device kernel from a registered host range "
                                         "through their addresses (no staging copy on the CPU); bound by the link as a kernel sees it",
                    "output": "TRXD v1 datagrams (160 B/burst) + 32 B result records",
                    "note": "pinned staging, one stream per slot; PCIe-inclusive rate, never `value`"}
        pipe.close()

    return exact_ms, mixed_s, mixed_detected, host_fed


PRECONDITION_S = 0.2


def read_sclk(out, device_index):
    """Current shader clock (MHz) of the device as rocm-smi reports it; {} left untouched when the tool is missing or slow."""
    import re
    import shutil
    import subprocess
    exe = shutil.which("rocm-smi") or "/opt/rocm/bin/rocm-smi"
    try:
        time.sleep(0.25)                                           # let the launches settle in
        r = subprocess.run([exe, "-d", str(device_index), "--showclocks"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, timeout=4.0)
        m = re.search(r"sclk clock level:\s*\d+:\s*\((\d+)Mhz\)", r.stdout)
        if m:
            out["sclk_mhz"] = int(m.group(1))
    except Exception:
        pass


def warm_clocks(fn, seconds=PRECONDITION_S):
    """Untimed launches of `fn` for `seconds`: the GPU's clocks need tens of milliseconds of load to settle (a leg that
    follows synthetic-data generation or the CPU baseline otherwise starts on idle clocks and reads 4-6 % low)."""
    import torch
    t0 = time.perf_counter()
    k = 0
    while True:
        fn()
        k += 1
        if k % 4 == 0:
            torch.cuda.synchronize()
            if time.perf_counter() - t0 >= seconds:
                break
    torch.cuda.synchronize()
    return k


def timed_passes(fn, shard, dev, world, passes=5):
    """Wall time of `passes` calls of fn, barrier + synchronize on both sides, max over ranks; plus the mean HIP-event time."""
    import torch
    warm_clocks(fn)
    shard.barrier()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(passes)]
    t0 = time.perf_counter()
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    shard.barrier()
    wall = shard.max_over_ranks(time.perf_counter() - t0, dev if shard.backend_name() else None)
    return wall, sum(a.elapsed_time(b) for a, b in ev) / passes


def config_legs(args, trx, synth, shard, n, dev, rank, world):
    """Driver-timed numbers for the other BASELINE.json configs (never `value`): configs[0] geometry, configs[2] (RACH and
    EXT_RACH), configs[3] (multi-ARFCN front end, alone and with the per-channel detector behind it) and -- for N > 1 -- the
    strong-scaling form of configs[4] (one fixed 8M-burst batch, contiguous shards, osmo_trx_amd.shard.shard_range)."""
    import numpy as np
    import torch
    from osmo_trx_amd import trxhip
    out = {}
    want = set(("c0", "c2", "c3") + (("strong",) if world > 1 else ())) if args.legs == "all" else set(args.legs.split(","))
    results = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    soft = torch.empty((n, 148), dtype=torch.float32, device=dev)

    def roof(bytes_per_pass, ms):
        gbs = bytes_per_pass / (ms * 1e-3) / 1e9
        return {"achieved_GBps": round(gbs, 1), "frac": round(gbs / HBM_PEAK_GBS, 4)}

    def pull_leg(key, workload, iq, params, burst_len, sps=4):
        dp = trx.params_tensor(params)
        # (the caller's copy of the slot types -> the TRXHIP_FLAG_FEW_NB_SLOTS hint, as the host pipe gives it; worked out once)
        hint = trxhip.few_nb_hint(params)
        wall, ms = timed_passes(lambda: trx.detect_demod(iq, dp, sps=sps, soft_stride=148, slice_bits=True, results=results,
                                                         soft=soft, hint=hint), shard, dev, world)
        det = int((trx.results_to_numpy(results)["rc"] > 0).sum())
        out[key] = {"workload": workload, "mbursts_per_s_all_gpus": round(5 * n * world / wall / 1e6, 2),
                    "kernel_ms": round(ms, 4), "detected_fraction": round(det / n, 4),
                    "roofline": roof(n * (burst_len * 4 + 8 + 32 + 592), ms)}

    if "c0" in want:
        # configs[0]: the reference's CPU-runnable case (1 SPS, TSC 0); on the GPU it is the generic kernel's geometry
        iq, p, _ = synth.make_normal_bursts(n, dev, 1, seed=synth.SEED + 11 + 1000003 * rank, tsc=0, burst_len=156)
        pull_leg("configs[0]", "normal bursts, 1 SPS, 156 samples, TSC 0, max_toa 3 (the reference's generic-C case; GPU: "
                 "burst_pull_kernel<1,...>)", iq, p, 156, sps=1)
        del iq
    if "c2" in want:
        # configs[2]: access bursts
        iq, p, _ = synth.make_access_bursts(n, dev, seed=synth.SEED + 1 + 1000003 * rank)
        pull_leg("configs[2]", "RACH bursts, 4 SPS, max_toa 63 (detectRACHBurst: 40 taps x 79 lags)", iq, p, 625)
        del iq
        iq, p, _ = synth.make_access_bursts(n, dev, seed=synth.SEED + 21 + 1000003 * rank, ext=True)
        pull_leg("configs[2]_ext_rach", "EXT_RACH bursts (TS0/1/2 tried in turn), max_toa 63", iq, p, 625)
        del iq
    del results, soft
    if "c3" in want:
        config3_leg(trx, synth, shard, dev, rank, world, out, roof)
    if "strong" in want:
        strong_leg(trx, synth, shard, dev, rank, world, out)
    return out


def config3_leg(trx, synth, shard, dev, rank, world, out, roof):
    import numpy as np
    import torch
    from osmo_trx_amd import trxhip
    if True:
        # configs[3]: 4-ARFCN front end over ~256k Channelizer blocks (a 416-timeslot, 3-carrier wideband capture repeated; the
        # synthesis is circular, so the tiled stream is continuous), then the detector on each carrier's channel stream
        tile_slots, reps = 52 * 8, 262
        wide1, nb1, _, tsc1 = synth.make_multi_arfcn_wideband(tile_slots, dev, seed=synth.SEED + 5 + rank)
        wide = wide1.repeat(reps, 1).contiguous()
        nb, n_slots = nb1 * reps, tile_slots * reps
        fe = trxhip.RxFrontEnd(trx)
        chan = [torch.empty((4, nb * 192 // 48 * 65), dtype=torch.complex64, device=dev)]   # (allocated once: not part of a pass)

        def front():
            fe.pull(wide, nb, out=chan[0])

        wall_f, ms_f = timed_passes(front, shard, dev, world)
        pp = np.zeros(n_slots, dtype=trxhip.PARAMS_DTYPE)
        pp["type"], pp["tsc"], pp["max_toa"] = 1, np.tile(tsc1, reps), 20
        dpp = trx.params_tensor(pp)
        res_c = torch.empty((n_slots, 32), dtype=torch.uint8, device=dev)
        soft_c = torch.empty((n_slots, 148), dtype=torch.float32, device=dev)
        found = [0, 0]

        def front_and_detect():
            front()
            for k in (0, 1, 3):                                     # the three carriers (filterbank channels 0, 1, 3)
                trx.detect_demod(chan[0][k].view(n_slots, 625), dpp, sps=4, soft_stride=148, slice_bits=True, results=res_c, soft=soft_c)

        wall_e, ms_e = timed_passes(front_and_detect, shard, dev, world, passes=3)
        found = int((trx.results_to_numpy(res_c)["rc"] > 0).sum())
        n_out = nb * 192 // 48 * 65
        fe_bytes = nb * 768 * 4 + 4 * n_out * 8     # wideband in, resampled out (the channel-rate streams stay on the chip since round 3)
        out["configs[3]"] = {
            "workload": f"4-ARFCN Channelizer(4,192,16) + Resampler(65,48) in one pass (frontend_fused_kernel) over {nb} blocks of 768 "
                        f"wideband int16 samples per GPU (streaming, carried history), then detect+demod of the {3 * n_slots} timeslots of the 3 carriers",
            "front_end_mblocks_per_s_all_gpus": round(5 * nb * world / wall_f / 1e6, 2), "front_end_ms": round(ms_f, 4),
            "front_end_roofline": roof(fe_bytes, ms_f),
            "with_per_channel_detect_mblocks_per_s_all_gpus": round(3 * nb * world / wall_e / 1e6, 2),
            "with_per_channel_detect_ms": round(ms_e, 4),
            "with_per_channel_detect_roofline": roof(fe_bytes + 3 * n_slots * (625 * 8 + 8 + 32 + 592), ms_e),
            "detected_fraction_last_carrier": round(found / n_slots, 4)}
        fe.close()
        del wide, wide1, chan, res_c, soft_c



def strong_leg(trx, synth, shard, dev, rank, world, out):
    import torch
    # configs[4], strong scaling: ONE fixed global batch of 8M mixed bursts, rank r owns shard_range(8M, r, N)
    if True:
        total = int(os.environ.get("TRXHIP_BENCH_STRONG_TOTAL", 8 << 20))     # (env: tests shrink the fixed batch)
        # the generator starts a shard on a multiple of 8 * chunk only: round the shard edges to that (any N, also 3, 5, 6, 7),
        # with a smaller generator chunk when the batch is too small for 65536-burst chunks on every rank
        chunk = 65536
        while chunk > 512 and 8 * chunk * world > total:
            chunk //= 2
        lo, hi = shard.shard_range_aligned(total, rank, world, 8 * chunk)
        m = hi - lo
        if m <= 0:
            raise SystemExit(f"strong leg: {total} bursts do not split over {world} ranks in blocks of {8 * chunk}")
        iq, p = synth.make_mixed_bursts(m, dev, seed=synth.SEED + 2, chunk=chunk, offset=lo)
        dp = trx.params_tensor(p)
        res_s = torch.empty((m, 32), dtype=torch.uint8, device=dev)
        soft_s = torch.empty((m, 148), dtype=torch.float32, device=dev)
        wall, ms = timed_passes(lambda: trx.detect_demod(iq, dp, sps=4, soft_stride=148, slice_bits=True, results=res_s,
                                                         soft=soft_s), shard, dev, world, passes=3)
        det = shard.sum_over_ranks(int((trx.results_to_numpy(res_s)["rc"] > 0).sum()), dev if shard.backend_name() else None)
        out["configs[4]_strong"] = {
            "workload": f"BASELINE.json configs[4]: ONE fixed batch of {total} mixed bursts (7:1 NB:RACH), contiguous shard "
                        f"[N*r/G, N*(r+1)/G) per rank with the edges rounded down to {8 * chunk} bursts, no data-path collective",
            "scaling": "strong",
            "global_bursts": total, "bursts_this_rank": m, "mbursts_per_s_all_gpus": round(3 * total / wall / 1e6, 2),
            "ms_per_pass": round(wall / 3 * 1e3, 4), "detected_fraction": round(det / total, 4)}
        del iq, res_s, soft_s


DUMP_SAMPLE = 65536            # bursts written by --dump-outputs: 65536 x 148 float32 soft bits = 38.8 MB, results ~2.4 MB
DUMP_SEED = 20240611


def dump_outputs(out_dir, trx, results, soft):
    """What a caller of the timed path receives -- the result records (one .npy per field) and the soft bits -- for a fixed,
    seeded sample of the batch's bursts (all of them when the batch is small), as float32 (float fields) or float64
    (integer fields, exact).  burst_index.npy says which bursts were sampled."""
    import numpy as np
    import torch
    n = results.shape[0]
    idx = np.arange(n) if n <= DUMP_SAMPLE else np.sort(np.random.default_rng(DUMP_SEED).choice(n, DUMP_SAMPLE, replace=False))
    sel = torch.from_numpy(idx).to(results.device)
    rec = trx.results_to_numpy(results[sel])
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "burst_index.npy"), idx.astype(np.float64))
    for name in rec.dtype.names:
        col = rec[name]
        np.save(os.path.join(out_dir, f"{name}.npy"), col.astype(np.float32 if col.dtype.kind == "f" else np.float64))
    np.save(os.path.join(out_dir, "soft.npy"), soft[sel].cpu().numpy().astype(np.float32))


def free_port():
    import socket
    so = socket.socket()
    so.bind(("127.0.0.1", 0))
    port = so.getsockname()[1]
    so.close()
    return port


def spawn_ranks(n):
    """`python bench.py --gpus N` with no torchrun environment: start the N ranks ourselves, one child process per GPU
    (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* as torch.distributed.run would set them), and pass rank 0's JSON line
    through.  The parent never touches the GPU (torch.cuda.device_count() does not initialise it): nothing that has
    made a HIP call is ever re-executed.  A rank that dies takes the others with it (their exact PIDs)."""
    import subprocess
    # (no device count here: on ROCm torch.cuda.device_count() falls back to hipGetDeviceCount() -- a HIP call in the launcher --
    # when amdsmi is unavailable; each rank reports a missing device itself)
    port = free_port()
    procs = []
    for r in range(n):
        # (HSA_ENABLE_IPC_MODE_LEGACY=0: the hosts of this pool support dmabuf IPC only; RCCL needs it for its peer buffers)
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), TRXHIP_BENCH_LAUNCHER="bench.py self-spawn")
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    rc = 0
    pending = list(procs)
    try:
        while pending:
            for p in list(pending):
                try:
                    r = p.wait(timeout=0.5)
                except subprocess.TimeoutExpired:
                    continue
                pending.remove(p)
                if r != 0 and rc == 0:
                    rc = r
                    for q in pending:                                # one rank failed: the others would wait in a collective
                        q.terminate()
    finally:
        # interrupted (or an exception above): do not leave ranks waiting in a collective -- their exact PIDs, nothing else
        for q in pending:
            if q.poll() is None:
                q.terminate()
        for q in pending:
            try:
                q.wait(timeout=5.0)
            except subprocess.TimeoutExpired:
                q.kill()
    return rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bursts", type=int, default=1 << 20, help="bursts per GPU per step")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-host-fed", action="store_true")
    ap.add_argument("--main-only", action="store_true",
                    help="profiling runs: only the timed configs[1] leg (no exact / mixed / host-fed side legs, no CPU baseline), "
                         "so that every launch of the hot kernel in a rocprofv3 trace is the one `value` is measured on")
    ap.add_argument("--cpu-sample", type=int, default=0, help="bursts for the CPU baseline (0 = auto)")
    ap.add_argument("--legs", default="all", help="which other_configs legs run: all | none | comma list of c0,c2,c3,strong "
                                                  "(strong = configs[4]'s fixed 8M batch; default only when N > 1)")
    ap.add_argument("--sustain-seconds", type=float, default=1.0,
                    help="length of the sustained leg (back-to-back launches behind the timed region; 0 = skip)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned (a fixed, seeded sample of rank 0's "
                         "bursts: every result field and the soft bits) as DIR/<name>.npy, for output-by-output comparison of builds")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:             # plain `python bench.py --gpus N`: launch the ranks here
        raise SystemExit(spawn_ranks(args.gpus))

    import numpy as np
    import torch
    from osmo_trx_amd import TrxHip, synth, shard

    rank, local_rank, world = shard.init_distributed()
    if world != args.gpus and world > 1:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: osmo_trx_amd has no CPU path")
    if os.environ.get("TRXHIP_ONE_DEVICE"):              # test hook: every rank on cuda:0 (with TRXHIP_DIST_BACKEND=gloo)
        local_rank = 0
    if local_rank >= torch.cuda.device_count():
        raise SystemExit(f"rank {rank}: LOCAL_RANK {local_rank} but this node shows {torch.cuda.device_count()} GPU(s) "
                         "(TRXHIP_ONE_DEVICE=1 with TRXHIP_DIST_BACKEND=gloo runs every rank on cuda:0: tests only)")
    dev = f"cuda:{local_rank}"
    torch.cuda.set_device(local_rank)

    # tables: generated on rank 0, RCCL-broadcast, checksum-verified, adopted on every rank
    blob = shard.broadcast_tables(dev if shard.backend_name() else None)
    trx = TrxHip(local_rank, tables_blob=blob)

    n = args.bursts
    iq, params, _ = synth.make_normal_bursts(n, dev, 4, seed=synth.SEED + 1000003 * rank)
    d_params = trx.params_tensor(params)
    results = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    soft = torch.empty((n, 148), dtype=torch.float32, device=dev)

    def step(exact=False):
        # default flags = what a deployment runs: vectorSlicer applied, fused demodulator
        trx.detect_demod(iq, d_params, sps=4, soft_stride=148, slice_bits=True, results=results, soft=soft, exact=exact)

    precond = warm_clocks(step)                                   # untimed, before the W warm-up steps: clock settling (see warm_clocks)
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    shard.barrier()
    torch.cuda.synchronize()

    # HIP events on the stream the C ABI launches on (torch's current stream is passed down): ONE pair around the K launches --
    # an event between two launches is a marker the next kernel's dispatch waits behind (5-8 us of idle GPU per step, which the
    # K back-to-back launches of a deployment do not have); the kernel's average duration is the span / K, launch gaps included
    ev_a, ev_b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    ev_a.record()
    for _ in range(args.steps):
        step()
    ev_b.record()
    torch.cuda.synchronize()
    shard.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    elapsed = shard.max_over_ranks(elapsed, dev if shard.backend_name() else None)
    kernel_ms = ev_a.elapsed_time(ev_b) / max(1, args.steps)
    kernel_ms = shard.max_over_ranks(kernel_ms, dev if shard.backend_name() else None)
    if args.dump_outputs and rank == 0:
        # before anything else reuses `results` / `soft`: they still hold what the last timed step computed
        dump_outputs(args.dump_outputs, trx, results, soft)

    # sustained leg (not `value`): >= --sustain-seconds of back-to-back launches of the same step, queued without a host
    # synchronisation in between, so that the 20-step timed region can be read against a second of continuous load
    sustained = None
    if args.sustain_seconds > 0:
        k_sus = max(args.steps, int(args.sustain_seconds * 1.05 / max(kernel_ms * 1e-3, 1e-6)) + 1)
        # the shader clock while the kernel runs, read once by rocm-smi from a side thread (rank 0): the boxes of a pool differ --
        # round 4 met one that ran every kernel at half clock -- and a reader of the line should see that next to the rate
        clock = {}
        watcher = None
        if rank == 0:
            import threading
            watcher = threading.Thread(target=read_sclk, args=(clock, local_rank), daemon=True)
        shard.barrier()
        torch.cuda.synchronize()
        t0s = time.perf_counter()
        if watcher:
            watcher.start()
        for _ in range(k_sus):
            step()
        torch.cuda.synchronize()
        t_sus = time.perf_counter() - t0s
        if watcher:
            watcher.join(timeout=5.0)
        shard.barrier()
        t_sus = shard.max_over_ranks(t_sus, dev if shard.backend_name() else None)
        sustained = {"seconds": round(t_sus, 3), "launches": k_sus, "mbursts_per_s_all_gpus": round(n * world * k_sus / t_sus / 1e6, 3),
                     "ms_per_step": round(t_sus / k_sus * 1e3, 4), "sclk_mhz_under_load": clock.get("sclk_mhz"),
                     "note": "back-to-back launches behind the timed region, no host synchronisation in between; never `value`"}

    # who ran: every rank's device, gathered over the same backend the tables were broadcast on
    props = torch.cuda.get_device_properties(local_rank)
    me = f"rank {rank}: cuda:{local_rank} {props.name} {getattr(props, 'gcnArchName', '')} pci {getattr(props, 'pci_bus_id', '?')}"
    devices = shard.gather_strings(me, dev if shard.backend_name() else None)
    backend = shard.backend_name()

    r = trx.results_to_numpy(results)
    detected = int((r["rc"] > 0).sum())
    ns = args.cpu_sample or min(n, max(8192, 4096 * usable_cores()))
    iq_cpu_sample = iq[:ns].cpu().numpy() if (rank == 0 and world == 1 and not args.no_cpu_baseline and not args.main_only) else None

    side = not args.main_only
    exact_ms = mixed_s = None
    mixed_detected = 0
    host_fed = None
    if side:
        exact_ms, mixed_s, mixed_detected, host_fed = side_legs(args, trx, synth, shard, step, iq, n, dev, rank, world, results, soft)
    del iq
    legs = {}
    if side and args.legs != "none":
        del results, soft
        legs = config_legs(args, trx, synth, shard, n, dev, rank, world)

    if rank == 0:
        total_bursts = n * world * args.steps
        value = total_bursts / elapsed / 1e6
        achieved = BYTES_PER_BURST * n / (kernel_ms * 1e-3) / 1e9
        # PMC counters are a recorded profile (separate --pmc passes cannot run inside this command): replayed only while the hot
        # kernels' sources still hash to what the profile was measured on (osmo_trx_amd/srchash.py), else null with the reason
        from osmo_trx_amd.srchash import replay_counters
        traffic = compute = None
        j, traffic_source = replay_counters(os.path.join(ROOT, "profiles", "pmc_traffic.json"))
        if j is not None:
            traffic = j["hbm_bytes_per_burst"] * n
            traffic_source = ("recorded PMC profile, not this run: profiles/pmc_traffic.json (" + str(j.get("tag", "?")) + ", kernel sources " +
                              str(j.get("source_hash")) + " = the working tree: FETCH_SIZE x2 + WRITE_SIZE per burst, separate --pmc passes) "
                              "x bursts_per_launch")
            if "compute" in j:
                # what loads the kernel in practice: vector ALU and LDS (SQ counters of the same recorded profile)
                compute = dict(j["compute"], bound="valu + lds at the chip's power limit",
                               source="recorded SQ counter passes, not this run: profiles/" + str(j.get("tag", "?")) + "_sq_counters.json")
        out = {
            "metric": "Mbursts/s detect+demod (156.25 sym, 4 SPS)",
            "value": round(value, 4), "unit": "Mbursts/s",
            "n_gpus": world, "world": world, "backend": backend or "none (single process)",
            "launcher": os.environ.get("TRXHIP_BENCH_LAUNCHER") or ("torch.distributed.run / external" if world > 1 else "single process"),
            "devices": devices, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 4),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "config": {
                "workload": "BASELINE.json configs[1]: 1M normal bursts per GPU, 4 SPS (625 int16 IQ samples), "
                            "all 8 TSCs, max_toa 3, 5% noise-only, 1% clipped; IQ resident in HBM",
                "bursts_per_gpu": n, "global_bursts": n * world, "sps": 4, "burst_len": 625,
                "clock_preconditioning": f"{precond} untimed launches ({PRECONDITION_S * 1e3:.0f} ms) in front of the {args.warmup} warm-up steps, "
                                         "and in front of every side leg: the timed steps run on settled clocks",
                "parallelism": f"batch-sharded x{world} (no data-path collective; tables RCCL-broadcast once)",
                "detected_fraction": round(detected / n, 4),
                "demodulator": "fused delay-o-decimate composite filter, taps 6..29 of 35 (default since round 5; profiles/r05_fused_taps.txt: "
                               "max relative error of a soft value with |soft| >= 0.05: 6.1e-5, 26 / 28 taps measured at -1.6 % / -3.2 %); "
                               f"|soft - ref| <= {FUSED_SOFT_ATOL:g} * max(1, rms / (4 |amp|)), absolute on full scale 1 "
                               f"(include/trxhip.h: plain {FUSED_SOFT_ATOL:g} on every real detection, amplitude-scaled on noise "
                               "slots detected far below their samples' level)",
                "detector": "FAST (fused kernels, round 5): rc / TSC / TOA identical to the reference -- FMA interpolation rounds, every "
                            "early / late decision certified by a proven rounding margin or re-run in the reference's operand order "
                            f"(0.5 % of detections); amp within {FAST_AMP_RTOL:g} relative (measured 5e-7), C/I within "
                            "1e-4 + 1.4e-5 (1 + 10^(ci/10)) dB; TRXHIP_FLAG_EXACT_DEMOD = the bit-exact kernel",
                "sustained": sustained,
                "exact_demod_mbursts_per_gpu": round(n / exact_ms / 1e3, 2) if side else None,
                "mixed_7to1_nb_rach": ({"workload": "BASELINE.json configs[4] per-GPU share: 7:1 NB:RACH, RACH max_toa 63",
                                        "mbursts_per_s_all_gpus": round(5 * n * world / mixed_s / 1e6, 3),
                                        "detected_fraction": round(mixed_detected / n, 4)} if side else None),
                "host_fed": host_fed,
                "other_configs": legs or None,
            },
            "roofline": {
                # `bound` names the roofline the fraction is priced against (the measurement contract: HBM bytes); what limits
                # the kernel in practice is in `compute` -- the vector ALU's issue rate, not HBM
                "bound": "hbm", "bound_note": "vector ALU + LDS in practice, at the chip's power limit (see compute, and config.sustained.sclk_mhz_under_load "
                                              "of 2400 MHz): `bound` names the roofline `frac` is priced against",
                "achieved": round(achieved, 3), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": round(achieved / HBM_PEAK_GBS, 6), "traffic": traffic, "traffic_source": traffic_source,
                "compute": compute,
                "kernel": "nb_pull4_kernel", "kernel_ms": round(kernel_ms, 4),
                "kernel_ms_note": "HIP events around the K timed steps / K: one step = the normal-burst kernel + the general kernel over the "
                                  "list it leaves behind (empty for this workload: returns at once), launch gaps included; the rocprofv3 "
                                  "kernel-trace average of nb_pull4_kernel in the same command is the pure kernel duration",
                "algorithmic_bytes_per_burst": BYTES_PER_BURST, "bursts_per_launch": n,
            },
        }
        if world == 1 and not args.no_cpu_baseline and not args.main_only:
            out["cpu_baseline"] = cpu_baseline(iq_cpu_sample, params[:ns])
        print(json.dumps(out), flush=True)

    if shard.backend_name():
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
