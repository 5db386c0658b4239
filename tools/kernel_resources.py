"""Per-kernel resources of two builds of one HIP source, side by side: VGPRs, AGPRs, SGPRs, scratch bytes, LDS bytes, occupancy
(waves per SIMD) and instruction count of every kernel, and whether the two instruction streams are the same (labels renumbered).

    hipcc -O3 -std=c++17 -ffp-contract=off --offload-arch=gfx950 --cuda-device-only -S csrc/fb_qnet.hip -o new.s     (and the parent's)
    python tools/kernel_resources.py parent.s new.s > profiles/NAME.txt

Needs c++filt on the PATH for the kernel names."""
import re, sys, subprocess
def parse(path):
    txt = open(path).read()
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", txt, re.S):
        name, body = m.group(1), m.group(2)
        g = lambda k: int(re.search(r"\.amdhsa_%s (\d+)" % k, body).group(1))
        out[name] = dict(lds=g("group_segment_fixed_size"), scratch=g("private_segment_fixed_size"), vgpr_next=g("next_free_vgpr"), agpr_off=g("accum_offset"))
    # function bodies: text between "name:" label and ".Lfunc_end"
    bodies = {}
    for name in out:
        m = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:" % re.escape(name), txt, re.S | re.M)
        b = m.group(1)
        info = re.search(r"; TotalNumSgprs: (\d+)\n; NumVgprs: (\d+)\n; NumAgprs: (\d+)\n; TotalNumVgprs: (\d+)\n; ScratchSize: (\d+)\n(?:.*\n)*?; Occupancy: (\d+)", txt[m.end():m.end()+6000])
        out[name].update(sgpr=int(info.group(1)), vgpr=int(info.group(2)), agpr=int(info.group(3)), scratch2=int(info.group(5)), occ=int(info.group(6)))
        code = [l.split(";")[0].strip() for l in b.splitlines()]
        code = [re.sub(r"\.LBB\d+_", ".LBB_", l) for l in code if l and not l.startswith(".")]
        bodies[name] = code
    return out, bodies
dem = lambda n: subprocess.run(["c++filt", n], capture_output=True, text=True).stdout.strip().replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
pa, pb = parse(sys.argv[1]); na, nb = parse(sys.argv[2])
print("# per-kernel resources of csrc/fb_qnet.hip for gfx950 (hipcc -O3 -ffp-contract=off), parent commit against this tree")
print("# kernel | parent: vgpr agpr sgpr scratch lds occupancy instructions | new: the same | machine code identical")
same = diff = 0
for n in sorted(set(pa) | set(na), key=dem):
    f = lambda a, b, n=n: ("%4d %4d %4d %5d %6d %2d %6d" % (a[n]["vgpr"], a[n]["agpr"], a[n]["sgpr"], a[n]["scratch"], a[n]["lds"], a[n]["occ"], len(b[n]))) if n in a else "   -    -    -     -      -  -      -"
    ident = n in pa and n in na and pb[n] == nb[n]
    if n in pa and n in na: same += ident; diff += not ident
    print(f"{dem(n):60s} | {f(pa, pb)} | {f(na, nb)} | {'yes' if ident else ('NEW' if n not in pa else 'NO')}")
print(f"# kernels in both: {same + diff}, identical instruction streams: {same}, different: {diff}")
