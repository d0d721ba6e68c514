"""Cost of one mmd_kv_drop at the 7B bf16 arena (28 layers, 4 kv heads, head_dim 128), beside hipMemcpyAsync device-to-device of the same byte count.

    python tools/kv_drop_bench.py [--out FILE.json]

The arena is declared live with mmd_kv_debug_set_len (contents are whatever the pages hold: the move is the same traffic); no weights are loaded.  Bytes moved =
tokens behind the span x 256 bytes x 112 (layer, kv head) rows x 2 (K and V), counted once (each is read once and written once)."""
import argparse, ctypes as C, json, os, sys
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--iters', type=int, default=5)
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
    for behind in (15_000, 100_000):
        for delta in (10, 1300):
            n = sink + delta + behind
            nbytes = behind * tok * rows * 2
            src = torch.empty(nbytes, dtype=torch.uint8, device='cuda'); dst = torch.empty_like(src)
            t_drop, t_copy = [], []
            for it in range(a.iters + 1):
                check(lib().mmd_kv_debug_set_len(h, n), m._ctx, 'set_len')
                m._bind_stream()
                st = torch.cuda.current_stream()
                e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
                e[0].record(st)
                check(lib().mmd_kv_drop(h, sink, sink + delta), m._ctx, 'mmd_kv_drop')
                e[1].record(st)
                e[2].record(st)
                assert hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, 3, st.cuda_stream) == 0
                e[3].record(st)
                st.synchronize()
                assert int(lib().mmd_kv_len(h)) == n - delta
                check(lib().mmd_stream_reset(h), m._ctx, 'reset')
                if it:          # (the first round maps the pages)
                    t_drop.append(e[0].elapsed_time(e[1])); t_copy.append(e[2].elapsed_time(e[3]))
            del src, dst
            md, mc = sorted(t_drop)[len(t_drop) // 2], sorted(t_copy)[len(t_copy) // 2]
            rec = dict(tokens_behind=behind, delta=delta, bytes_moved=nbytes, drop_ms=md, drop_GBps=nbytes / md / 1e6, memcpy_ms=mc, memcpy_GBps=nbytes / mc / 1e6,
                       ratio_drop_over_memcpy_time=md / mc, drop_ms_all=t_drop, memcpy_ms_all=t_copy)
            print(json.dumps(rec), flush=True)
            out.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
