#!/usr/bin/env python3
"""What a break costs the large-frame stride decode (decode_large: k_unmask_inplace<64, 1, true> ->
k_large_fix), beside the k_plan-first path (UVHTTP_WS_LARGE_SPEC=0) in the same process.

  python tools/large_break_probe.py [n_frames [payload]]        (default 65536 x 65536: C3)

The generated wire's first header bytes are rewritten on the device: a lone CONTINUATION at the
first, the middle or the last frame (everything from it on must be restored), or a valid
fragmented message in the middle (no failure: every round of k_large_fix's scan runs, nothing is
restored).  Per case and engine: the median step of ROUNDS x K calls (events, stamps off), then
the stamped kernel durations and gaps of 16 more calls.  The last rows answer whether stamps slow
the payload kernel: its stamped median with the stamped calls issued right after the ring's
clearing copy, and after 300 more calls."""
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

import uvhttp_amd as U  # noqa: E402
from bench import summarize_stamps  # noqa: E402

ROUNDS, K = 5, 20


def engine(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return U.GpuEngine(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
    plen = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
    engs = [("large", engine({"UVHTTP_WS_LARGE_SPEC": "1"})), ("k_plan first", engine({"UVHTTP_WS_LARGE_SPEC": "0"}))]
    stride = U.gen_frame_stride(plen)
    wl = stride * n
    wire = torch.empty(wl + 64, dtype=torch.uint8, device="cuda")
    engs[0][1].gen_frames(wire, n, plen, 7, opcode0=2, fragmented=False)
    b0 = int(wire[0].item())
    st = torch.cuda.current_stream()
    outs = [e.alloc_outputs(n) for _, e in engs]

    def run(k):
        desc, summ = outs[k]
        engs[k][1].decode_inplace(wire, n, stride=stride, max_message_size=256 << 20, wire_len=wl,
                                  desc=desc, summary=summ, stream=st)

    def timeline(k, warm):
        e = engs[k][1]
        e.set_stamps(True)
        e.read_stamps()
        for _ in range(warm):
            run(k)
        torch.cuda.synchronize()
        if warm:
            e.read_stamps()
        for _ in range(16):
            run(k)
        torch.cuda.synchronize()
        tl = summarize_stamps(e.read_stamps())
        e.set_stamps(False)
        return tl

    cases = [("clean", {}), ("lone continuation at frame 0", {0: 0x80}),
             ("lone continuation at the middle frame", {n // 2: 0x80}),
             ("lone continuation at the last frame", {n - 1: 0x80}),
             ("valid fragmented message in the middle", {n // 2: b0 & 0x7F, n // 2 + 1: 0x80})]
    for name, edits in cases:
        for i in edits:
            wire[i * stride] = edits[i]
        torch.cuda.synchronize()
        for k, (ename, e) in enumerate(engs):
            steps = []
            for r in range(ROUNDS + 1):
                for _ in range(3):
                    run(k)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(st)
                for _ in range(K):
                    run(k)
                b.record(st)
                b.synchronize()
                if r:
                    steps.append(a.elapsed_time(b) / K * 1e3)
            s = e.read_summary(outs[k][1])
            tl = timeline(k, 3)
            print(f"{name:42s} {ename:13s} step {statistics.median(steps):8.1f} us ({min(steps):.1f} .. {max(steps):.1f})"
                  f"  delivered {s['n_delivered']} status {s['status']}  stamps: {tl['kernels_us']} gaps {tl['gaps_us']}",
                  flush=True)
        for i in edits:
            wire[i * stride] = b0
    torch.cuda.synchronize()
    for k, (ename, e) in enumerate(engs):
        for warm in (0, 3, 300):
            tl = timeline(k, warm)
            print(f"clean, stamped after {warm:3d} warm-up calls  {ename:13s} payload {tl['kernels_us'].get('payload')} us"
                  f"  chain {tl['chain_us']}  between calls {tl['gap_between_calls_us']}", flush=True)
    for _, e in engs:
        e.close()


if __name__ == "__main__":
    main()
