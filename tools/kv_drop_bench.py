"""Cost of one mmd_kv_drop at the 7B bf16 arena (28 layers, 4 kv heads, head_dim 128), beside hipMemcpyAsync device-to-device of the same byte count.

    python tools/kv_drop_bench.py [--out FILE.json] [--shift] [--reps N] [--spans M]

--shift: mmd_kv_drop_shift on the same span as well, the two calls alternating (in alternating order) on the same arena; the span of tests/test_gpu_kv_drop_trueshape.py
is added to the shapes.  --reps N: N calls between the two events of a timed window (the length is declared again in front of each: host bookkeeping, no launch), the
time reported per call.

--spans M: instead of the above, ONE mmd_kv_drop_spans over M evenly spread frame-sized (49-token) spans against M mmd_kv_drop calls over the same spans, last span
first (profiles/kv_drop_spans.md); the two alternate in one process, with 15 k and 100 k tokens behind the first span, plain and shifted, and ONE single drop of the
first span is timed in every round beside them (the single drop's payload rate at the same depth, in the same run).

The arena is declared live with mmd_kv_debug_set_len (contents are whatever the pages hold: the move is the same traffic); no weights are loaded.  Bytes moved =
tokens behind the span x 256 bytes x 112 (layer, kv head) rows x 2 (K and V), counted once (each is read once and written once)."""
import argparse, ctypes as C, json, os, sys
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--shift', action='store_true')
    ap.add_argument('--reps', type=int, default=1)
    ap.add_argument('--spans', type=int, default=0)
    a = ap.parse_args()
    from mmduet_amd._lib import lib, check
    from mmduet_amd.configuration_live import VideoHeadLiveLlavaQwenConfig
    from mmduet_amd.modeling_live import VideoHeadLiveLlavaQwenForCausalLM
    cfg = VideoHeadLiveLlavaQwenConfig(vocab_size=2048, num_hidden_layers=28, intermediate_size=256, vit_num_hidden_layers=2, vit_layers_removed=1,
                                       frame_num_tokens=49, frame_resolution=384, v_placeholder='<image>')
    m = VideoHeadLiveLlavaQwenForCausalLM(cfg, torch_dtype=torch.bfloat16, max_vit_batch=1, max_step_tokens=256, kv_initial_tokens=1024)
    c = m.config
    rows, tok = c.num_hidden_layers * c.num_key_value_heads, c.head_dim * 2
    assert (rows, tok) == (112, 256)
    hip = C.CDLL('libamdhip64.so')
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    cache = m.new_cache(1024)
    h = cache.arena.h
    sink, out = 20, []
    if a.spans > 0:
        return bench_spans(a, m, h, sink, rows, tok)
    calls = [('drop', lib().mmd_kv_drop)] + ([('drop_shift', lib().mmd_kv_drop_shift)] if a.shift else [])
    shapes = ([(1980, 1000)] if a.shift else []) + [(behind, delta) for behind in (15_000, 100_000) for delta in (10, 1300)]
    for behind, delta in shapes:
        n = sink + delta + behind
        nbytes = behind * tok * rows * 2
        src = torch.empty(nbytes, dtype=torch.uint8, device='cuda'); dst = torch.empty_like(src)
        t_drop, t_copy, t_shift = [], [], []
        for it in range(a.iters + 1):
            m._bind_stream()
            st = torch.cuda.current_stream()
            e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            for name, call in (calls if it % 2 == 0 else calls[::-1]):
                e[0].record(st)
                for _ in range(a.reps):
                    check(lib().mmd_kv_debug_set_len(h, n), m._ctx, 'set_len')
                    check(call(h, sink, sink + delta), m._ctx, name)
                e[1].record(st)
                st.synchronize()
                if it:
                    (t_drop if name == 'drop' else t_shift).append(e[0].elapsed_time(e[1]) / a.reps)
            e[2].record(st)
            assert hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, 3, st.cuda_stream) == 0
            e[3].record(st)
            st.synchronize()
            assert int(lib().mmd_kv_len(h)) == n - delta
            check(lib().mmd_stream_reset(h), m._ctx, 'reset')
            if it:          # (the first round maps the pages)
                t_copy.append(e[2].elapsed_time(e[3]))
        del src, dst
        md, mc = sorted(t_drop)[len(t_drop) // 2], sorted(t_copy)[len(t_copy) // 2]
        rec = dict(tokens_behind=behind, delta=delta, bytes_moved=nbytes, drop_ms=md, drop_GBps=nbytes / md / 1e6, memcpy_ms=mc, memcpy_GBps=nbytes / mc / 1e6,
                   ratio_drop_over_memcpy_time=md / mc, drop_ms_all=t_drop, memcpy_ms_all=t_copy, reps=a.reps)
        if a.shift:
            ms = sorted(t_shift)[len(t_shift) // 2]
            rec.update(drop_shift_ms=ms, drop_shift_GBps=nbytes / ms / 1e6, ratio_shift_over_drop_time=ms / md, drop_shift_ms_all=t_shift)
        print(json.dumps(rec), flush=True)
        out.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, 'w'), indent=1)


def bench_spans(a, m, h, sink, rows, tok):
    from mmduet_amd._lib import lib, check
    M, frame, out = a.spans, 49, []
    for behind in (15_000, 100_000):
        n = sink + behind
        step = behind // M
        spans = [(sink + i * step, sink + i * step + frame) for i in range(M)]          # evenly spread over what lies behind the sink
        flat = (C.c_int64 * (2 * M))(*[x for sp in spans for x in sp])
        moved_once = (behind - M * frame) * tok * rows * 2                              # every retained byte behind the first span, once
        moved_m = sum(n - b for _, b in spans) * tok * rows * 2                         # what M single drops move (each its whole tail), an upper figure: later drops see shorter tails
        for shift in (0, 1):
            one = lib().mmd_kv_drop_shift if shift else lib().mmd_kv_drop

            def many_calls():
                for f, t in reversed(spans):
                    check(one(h, f, t), m._ctx, 'drop')

            def one_call():
                check(lib().mmd_kv_drop_spans(h, C.cast(flat, C.c_void_p), M, shift), m._ctx, 'drop_spans')
            def single():          # ONE drop of the first span: the single drop's payload rate at this depth, in the same run
                check(one(h, *spans[0]), m._ctx, 'drop')
            t_one, t_many, t_single = [], [], []
            for it in range(a.iters + 1):
                m._bind_stream()
                st = torch.cuda.current_stream()
                for name, call in ((('one', one_call), ('many', many_calls)) if it % 2 == 0 else (('many', many_calls), ('one', one_call))):
                    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                    check(lib().mmd_kv_debug_set_len(h, n), m._ctx, 'set_len')
                    e[0].record(st)
                    call()
                    e[1].record(st)
                    st.synchronize()
                    assert int(lib().mmd_kv_len(h)) == n - M * frame
                    if it:          # (the first round maps the pages)
                        (t_one if name == 'one' else t_many).append(e[0].elapsed_time(e[1]))
                e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                check(lib().mmd_kv_debug_set_len(h, n), m._ctx, 'set_len')
                e[0].record(st)
                single()
                e[1].record(st)
                st.synchronize()
                if it:
                    t_single.append(e[0].elapsed_time(e[1]))
                check(lib().mmd_stream_reset(h), m._ctx, 'reset')
            ms1, single_bytes = sorted(t_single)[len(t_single) // 2], (n - spans[0][1]) * tok * rows * 2
            mo, mm = sorted(t_one)[len(t_one) // 2], sorted(t_many)[len(t_many) // 2]
            rec = dict(spans=M, span_tokens=frame, tokens_behind=behind, shift=bool(shift), bytes_moved_one_pass=moved_once, one_call_ms=mo, one_call_GBps=moved_once / mo / 1e6,
                       m_calls_ms=mm, m_calls_bytes_upper=moved_m, ratio_one_over_m_time=mo / mm, one_call_ms_all=t_one, m_calls_ms_all=t_many,
                       single_drop_ms=ms1, single_drop_bytes=single_bytes, single_drop_GBps=single_bytes / ms1 / 1e6, single_drop_ms_all=t_single)
            print(json.dumps(rec), flush=True)
            out.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
