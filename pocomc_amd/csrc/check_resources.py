"""Build-time check of the lane-per-walker sweep (csrc/maf_inverse_tri6.hip): its register-capped instances -- plain
inverse (FM = 0) with one subset, or two subsets and 16-bit helpers: __launch_bounds__(64 NW, 2) -- exist because
they run without AGPR copies and without scratch; a toolchain that spills them would be a silent regression of the hot
kernel of BASELINE configs 3 and 5.  Reads the compiler's -Rpass-analysis=kernel-resource-usage remarks and fails the
build if a capped instance uses scratch or accumulation registers.   python3 check_resources.py <remarks.txt>

python3 check_resources.py --no-scratch NAME[,NAME...] <remarks.txt>: the row kernels of the MCMC step (csrc/step.hip) are
one thread per walker with nothing to spill; prints the registers / LDS of every kernel whose name contains a NAME and fails
the build if one is missing or uses scratch."""
import re
import sys

name = re.compile(r"Function Name: (\S+)")
if sys.argv[1] == "--no-scratch":
    blocks = name.split(open(sys.argv[3]).read())[1:]
    field = lambda body, key: int(re.search(re.escape(key) + r": (\d+)", body).group(1))
    for want in sys.argv[2].split(","):
        hits = [(fn, body) for fn, body in zip(blocks[0::2], blocks[1::2]) if want in fn]
        if not hits:
            sys.exit(f"check_resources: no kernel named {want} in the remarks")
        for fn, body in hits:
            scratch = field(body, "ScratchSize [bytes/lane]")
            print(f"check_resources: {want}: VGPRs {field(body, ' VGPRs')}, AGPRs {field(body, 'AGPRs')}, SGPRs {field(body, 'TotalSGPRs')}, "
                  f"LDS {field(body, 'LDS Size [bytes/block]')} B/block, scratch {scratch} B/lane, "
                  f"occupancy {field(body, 'Occupancy [waves/SIMD]')} waves/SIMD")
            if scratch:
                sys.exit(f"check_resources: {want} uses {scratch} B/lane of scratch")
    sys.exit(0)
txt = open(sys.argv[1]).read()
inst = re.compile(r"maf_inverse_tri6_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)E")
blocks = name.split(txt)[1:]
bad, seen = [], 0
for fn, body in zip(blocks[0::2], blocks[1::2]):
    m = inst.search(fn)
    if not m:
        continue
    ns, fm, nw, hb = (int(v) for v in m.groups())
    capped = fm == 0 and (ns == 1 or (ns == 2 and hb != 0))
    if not capped:
        if fm == 0 and nw == 5:        # five wavefronts share four SIMDs: 256 registers by construction, reported only
            sc = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", body).group(1))
            if sc:
                print(f"check_resources: note: maf_inverse_tri6_kernel<{ns}, {fm}, {nw}, {hb}> uses {sc} B/lane of scratch")
        continue
    seen += 1
    scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", body).group(1))
    agpr = int(re.search(r"AGPRs: (\d+)", body).group(1))
    vgpr = int(re.search(r"\bVGPRs: (\d+)", body).group(1))
    if scratch or agpr or vgpr > 256:
        bad.append(f"maf_inverse_tri6_kernel<{ns}, {fm}, {nw}, {hb}>: VGPRs {vgpr}, AGPRs {agpr}, scratch {scratch} B/lane")
if not seen:
    sys.exit("check_resources: no capped instance of maf_inverse_tri6_kernel found in the remarks")
if bad:
    sys.exit("check_resources: register-capped instances spill:\n  " + "\n  ".join(bad))
print(f"check_resources: {seen} capped instances of maf_inverse_tri6_kernel: no scratch, no AGPRs")
