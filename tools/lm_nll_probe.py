#!/usr/bin/env python
"""Teacher-forced scoring at the 7B lm_head shape: the chunked path (mmd_op_lm_nll: GEMM into a <= 64 MiB fp32 workspace + streaming cross-entropy reduce per
vocabulary chunk) against the route that existed before it (mmd_op_gemm into a full [M, V] fp32 tensor, then torch.nn.functional.cross_entropy(reduction='none')).

python tools/lm_nll_probe.py [--rows 1274 4096] [--iters 5] [--rounds 3] [--out FILE.json]

bf16 context, random W [152064, 3584] and X [M, 3584], random labels.  Per route and M: wall time per call from HIP events (warm-up first, the two routes
alternating inside every round, the median round reported with the spread), torch.cuda.max_memory_allocated over the route's calls beyond the operands, and for
the chunked path the library's own workspace on top of it.  Both routes run the same GEMM kernel family (the fp32-output tile kernel; neither packs W).
Prints one JSON line per M; the record of a run is profiles/r07_lm_nll.md."""
import argparse, json, os, statistics, sys
import torch
import torch.nn.functional as F
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__)))); sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
from rawops import RawOps
from mmduet_amd._lib import lib, check
from mmduet_amd.modeling_live import _ptr

V, K = 152064, 3584
WS_MAX = 64 << 20
GEMM_LARGE = 3          # the 128-row tile kernel the automatic dispatch picks for an fp32-output GEMM at M >= 256, without mmd_op_gemm's per-call packing of W


def plan(M, max_rows):
    """row block, workspace bytes and automatic chunk width of lm_nll_run (mmduet_amd/csrc/model.hip) for M rows"""
    rows = min(M, max_rows, 32768)
    ws = min(WS_MAX, rows * (-(-V // 256) * 256) * 4)
    cw = min(V, ws // (rows * 4) // 256 * 256)
    return rows, ws, cw


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, nargs='+', default=[1274, 4096])
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--max-step-tokens', type=int, default=1530)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('lm_nll_probe needs the GPU: no time is reported without one')
    ops = RawOps(torch.bfloat16, max_step_tokens=a.max_step_tokens)
    g = torch.Generator(device='cuda').manual_seed(0)
    W = (torch.randn(V, K, generator=g, device='cuda') * 0.02).to(torch.bfloat16)
    results = []
    for M in a.rows:
        X = (torch.randn(M, K, generator=g, device='cuda') * 0.5).to(torch.bfloat16)
        labels = torch.randint(0, V, (M,), generator=g, device='cuda')
        nll = torch.empty(M, dtype=torch.float32, device='cuda')
        ops.m._bind_stream()

        def chunked():
            check(lib().mmd_op_lm_nll(ops.ctx, _ptr(X), _ptr(W), M, V, K, _ptr(labels), -100, 0, _ptr(nll), None), ops.ctx, 'mmd_op_lm_nll')
            return nll

        def full():
            Y = torch.empty(M, V, dtype=torch.float32, device='cuda')
            check(lib().mmd_op_gemm(ops.ctx, _ptr(X), _ptr(W), None, None, _ptr(Y), M, V, K, 0, 1, GEMM_LARGE), ops.ctx, 'mmd_op_gemm')
            return F.cross_entropy(Y, labels, reduction='none')

        peaks = {}
        for name, fn in (('chunked', chunked), ('full', full)):          # warm-up, and the peak allocation of one route at a time
            torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            out = fn(); out = fn(); torch.cuda.synchronize()
            peaks[name] = torch.cuda.max_memory_allocated() - base
            ref = out.clone() if name == 'full' else None
            if name == 'chunked':
                got = out.clone()
        agree = float((got - ref).abs().max())          # both routes see the same bf16-rounded logits of the same kernel: the streaming fp32 reduce against torch's
        tc, tf = [], []
        for _ in range(a.rounds):
            tc.append(timed(chunked, a.iters)); tf.append(timed(full, a.iters))
        rows, ws, cw = plan(M, a.max_step_tokens)
        r = dict(M=M, V=V, K=K, dtype='bf16', iters=a.iters, rounds=a.rounds,
                 chunked_ms=statistics.median(tc), chunked_ms_rounds=tc, full_ms=statistics.median(tf), full_ms_rounds=tf,
                 chunked_over_full=statistics.median(tc) / statistics.median(tf),
                 chunked_peak_torch_bytes=peaks['chunked'], chunked_library_workspace_bytes=ws, full_peak_torch_bytes=peaks['full'],
                 row_block=rows, auto_chunk_cols=cw, chunks=-(-V // cw), max_abs_difference_of_the_two_routes=agree)
        print(json.dumps(r), flush=True)
        results.append(r)
        del X, labels, nll, ref, got, out
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(results, open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
