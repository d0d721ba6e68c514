"""Rates of the snapshot paths at the 7B bf16 arena (28 layers, 4 kv heads, head_dim 128; 57 344 bytes of K and V per token), beside mmd_kv_stash of the same
token range -- the existing strided copy of the same bytes -- on the same machine in the same run.

    python profiles/kv_snapshot_bench.py [--tokens 16384] [--reps 20] [--staging-mb 256] [--out FILE.json]

Timed with device events on the model's stream, the four paths one after the other inside every repetition, one untimed repetition first:
  save    what kv_save enqueues without its host copies: mmd_kv_export chunk by chunk into the staging buffers;
  load    what kv_load enqueues without its host copies: mmd_kv_import chunk by chunk out of the staging buffers, into a second arena that was reset;
  fork    mmd_kv_fork of the whole context into that second arena;
  stash   mmd_kv_stash of [0, tokens) of the source arena.
The source arena is declared live with mmd_kv_debug_set_len (its pages hold zeros: a copy moves the same traffic); no weights are loaded.  Bytes = tokens x 57 344,
counted once (read once, written once)."""
import argparse, ctypes as C, json, os, sys
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tokens', type=int, default=16384)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--staging-mb', type=int, default=256)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from mmduet_amd._lib import lib, check
    from mmduet_amd.configuration_live import VideoHeadLiveLlavaQwenConfig
    from mmduet_amd.modeling_live import VideoHeadLiveLlavaQwenForCausalLM, snapshot_chunks, _ptr
    cfg = VideoHeadLiveLlavaQwenConfig(vocab_size=2048, num_hidden_layers=28, intermediate_size=256, vit_num_hidden_layers=2, vit_layers_removed=1,
                                       frame_num_tokens=49, frame_resolution=384, v_placeholder='<image>')
    m = VideoHeadLiveLlavaQwenForCausalLM(cfg, torch_dtype=torch.bfloat16, max_vit_batch=1, max_step_tokens=256, kv_initial_tokens=1024)
    c = m.config
    layers, nkv, d = c.num_hidden_layers, c.num_key_value_heads, c.head_dim
    token_bytes = 2 * layers * nkv * d * 2
    assert token_bytes == 57344
    n = a.tokens
    caches = m.new_cache(n), m.new_cache(n)          # (kept: an arena goes back to the pool with its last handle)
    src, dst = caches[0].arena.h, caches[1].arena.h
    check(lib().mmd_kv_debug_set_len(src, n), m._ctx, 'set_len')
    chunks = snapshot_chunks(n, token_bytes, a.staging_mb << 20)
    per = max(b - a_ for a_, b in chunks)
    sk = torch.zeros(layers * nkv * per * d, dtype=torch.bfloat16, device='cuda'); sv = torch.zeros_like(sk)
    m._bind_stream()
    st = torch.cuda.current_stream()

    def save():
        for a_, b in chunks:
            check(lib().mmd_kv_export(src, a_, b, _ptr(sk), _ptr(sv)), m._ctx, 'mmd_kv_export')

    def load():
        for a_, b in chunks:
            check(lib().mmd_kv_import(dst, _ptr(sk), _ptr(sv), b - a_), m._ctx, 'mmd_kv_import')

    def fork():
        check(lib().mmd_kv_fork(dst, src, n), m._ctx, 'mmd_kv_fork')

    def stash():
        check(lib().mmd_kv_stash(src, 0, n), m._ctx, 'mmd_kv_stash')
    paths = [('save', save), ('load', load), ('fork', fork), ('stash', stash)]
    ms = {k: [] for k, _ in paths}
    for rep in range(a.reps + 1):
        for name, fn in paths:
            check(lib().mmd_stream_reset(dst), m._ctx, 'reset')          # (the pages stay mapped: the first repetition maps them and allocates the stash)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st); fn(); e1.record(st)
            st.synchronize()
            if rep:
                ms[name].append(e0.elapsed_time(e1))
    nbytes = n * token_bytes
    p = torch.cuda.get_device_properties(0)
    rec = dict(device=p.name, arch=getattr(p, 'gcnArchName', ''), compute_units=p.multi_processor_count, tokens=n, bytes=nbytes, chunks=len(chunks), reps=a.reps)
    for name, t in ms.items():
        t = sorted(t)
        med = t[len(t) // 2]
        rec[name] = dict(median_ms=med, min_ms=t[0], max_ms=t[-1], GBps=nbytes / med / 1e6)
    for name in ('save', 'load', 'fork'):
        rec[name]['rate_over_stash'] = rec[name]['GBps'] / rec['stash']['GBps']
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(rec, open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
