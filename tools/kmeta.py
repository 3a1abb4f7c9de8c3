#!/usr/bin/env python3
"""Per-kernel register/LDS/scratch usage from a hipcc --cuda-device-only -S listing.

    python tools/kmeta.py file.s [substring] [--check]

--check: exit 1 when a listed kernel uses scratch, spills VGPRs or has more
than 128 VGPRs (the cap of the 16-wave kernels at 4 waves per SIMD).  The
unit-loop kernels of binary_gs.hip sit at 125-128 VGPRs and stay free of
scratch only by the opaque thread-id copies in binary_dev.hpp, so run

    hipcc -O3 -std=c++17 -Icsrc/include -Iinclude -x hip --offload-arch=gfx950 -munsafe-fp-atomics \\
      -ffp-contract=fast -DPGA_BIN_GS=8 --cuda-device-only -S csrc/kernels/binary_gs.hip -o gs8.s
    python tools/kmeta.py gs8.s binary_gen_tp --check

after a toolchain change (no GPU needed).
"""
import re
import sys

args = [a for a in sys.argv[1:] if a != "--check"]
check = "--check" in sys.argv[1:]
src = open(args[0]).read()
pat = args[1] if len(args) > 1 else ""
meta = src[src.index("amdhsa.kernels:"):]
bad = []
for ent in re.split(r"\n  - ", meta)[1:]:
    name = re.search(r"\.name:\s+(\S+)", ent)
    if not name or pat not in name.group(1):
        continue
    get = lambda k: (re.search(re.escape(k) + r":\s+(\d+)", ent) or [None, "?"])[1]
    print(f"{name.group(1)[:90]:90s} sgpr {get('.sgpr_count'):>4} vgpr {get('.vgpr_count'):>4} agpr {get('.agpr_count'):>3} "
          f"spill s/v {get('.sgpr_spill_count')}/{get('.vgpr_spill_count')} lds {get('.group_segment_fixed_size')} "
          f"scratch {get('.private_segment_fixed_size')}")
    num = lambda k: int(get(k)) if get(k) != "?" else 0
    if check and (num(".private_segment_fixed_size") > 0 or num(".vgpr_spill_count") > 0 or num(".vgpr_count") > 128):
        bad.append(name.group(1))
if check and bad:
    print(f"kmeta --check: {len(bad)} kernel(s) with scratch, VGPR spills or more than 128 VGPRs:", file=sys.stderr)
    for b in bad:
        print("  " + b, file=sys.stderr)
    sys.exit(1)
