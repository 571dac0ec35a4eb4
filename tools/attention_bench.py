#!/usr/bin/env python3
"""Time per launch of the split-precision attention kernel at the flagship shape (B = 508, L = 129, 12 heads:
attention_split_kernel<8,4,XKEY>), alone: mpreid_vit_attention on a seeded q | k | v buffer, hipEvents around each launch
(mpreid_profile_* hooks), all query tiles and the CLS tile only.

    python tools/attention_bench.py [tag]

With a timing-ablation build (MPREID_ABLATION=1 python mp-reid_amd/mpreid/build.py; MPREID_LIB=tools/ablation_lib/...
MPREID_ALLOW_ABLATION=1) MPREID_ATT_DBG selects what the kernel leaves out (csrc/attention.hip); the switch is latched per process, so
one process per value.  profiles/attention_split_ablation.log holds such a table."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mp-reid_amd")]
import torch  # noqa: E402

from mpreid import _lib, ops  # noqa: E402

B, L, H = 508, 129, 12


def main():
    tag = sys.argv[1] if len(sys.argv) > 1 else ""
    Lb = _lib.load()
    g = torch.Generator(device="cuda").manual_seed(3)
    qkv = torch.randn((B * L, 3 * 64 * H), generator=g, device="cuda") * 1.4
    out = torch.empty((B * L, 2 * 64 * H), dtype=torch.float16, device="cuda")
    for q_tiles in (0, 1):
        for _ in range(3):
            ops.vit_attention(qkv, B, L, H, q_tiles=q_tiles, out=out)
        torch.cuda.synchronize()
        Lb.mpreid_profile_reset()
        Lb.mpreid_profile_enable(1)
        for _ in range(20):
            ops.vit_attention(qkv, B, L, H, q_tiles=q_tiles, out=out)
        torch.cuda.synchronize()
        Lb.mpreid_profile_enable(0)
        ents = (_lib.ProfileEntry * 16)()
        n = Lb.mpreid_profile_query(ents, 16)
        for i in range(n):
            e = ents[i]
            if e.epilogue == 101:
                us = e.total_ms / e.launches * 1e3
                print("ATT_TIME %s dbg=%s q_tiles=%d launches=%d us_per_launch=%.1f GB/s=%.0f" % (
                    tag, os.environ.get("MPREID_ATT_DBG", "0"), q_tiles, e.launches, us, e.flops_total / e.launches / us / 1e3))


if __name__ == "__main__":
    main()
