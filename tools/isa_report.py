#!/usr/bin/env python3
"""profiles/polar_share_headline_isa.txt (boxtab_headline_isa.txt: the kernel before the second loop rendered groups of tiles
from one run of the angles; shared_rows_headline_isa.txt: before the second loop read its tile boxes from
a table; r03_headline_isa.txt: before the first loop rendered groups): what the shipped headline kernel is made of.
Compiles eu_render4.hip (which includes eu_render5.h) with -save-temps, reports registers, scratch and occupancy of the
degree-3 FAST instantiations - with the box table (the shipped form) and without (EU_HIP_BOXTAB=0, a refused table) -
takes eu_render5_kernel<3,3,SPHERICAL,FAST,BOXTAB> out of the ISA listing and
reports the code-object metadata, the instruction mix (whole kernel and per stage of the first loop's group of 16x16
tiles - the coordinate stage, once per group, and the member stage - cut at the stage's first characteristic instruction;
per stage of the second loop's position - once per position, per member, per pass - cut by the compiler's loop annotations,
with the scratch accesses that lie inside that loop), and - from the PMC record in profiles/ - the executed counts per tile.
usage: python tools/isa_report.py > profiles/polar_share_headline_isa.txt"""
import collections, os, re, subprocess, sys, tempfile, json

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "_Z17eu_render5_kernelILi3ELi3ELi0ELb1ELb1EEv"
tmp = tempfile.mkdtemp(prefix="isa_")
subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "--offload-arch=gfx950", "-ffp-contract=off", "-fPIC", "-std=c++17",
                       "-Wno-unused-function", "-Wno-pass-failed", "-save-temps=obj", "-c",
                       os.path.join(ROOT, "envutil_amd/csrc/eu_render4.hip"), "-o", os.path.join(tmp, "eu_render4.o")],
                      stderr=subprocess.DEVNULL)
lines = open(os.path.join(tmp, "eu_render4-hip-amdgcn-amd-amdhsa-gfx950.s")).read().split("\n")
s = next(i for i, l in enumerate(lines) if l.startswith(KERNEL))
e = next(i for i in range(s, len(lines)) if ".end_amdhsa_kernel" in lines[i])
body = lines[s:e]
ins = [(i, l.split()[0]) for i, l in enumerate(body) if re.match(r"^\s+[a-z]", l) and not l.strip().startswith(".")]
meta = [l.strip() for l in body if re.search(r"amdhsa_(next_free_vgpr|next_free_sgpr|group_segment_fixed_size|private_segment_fixed_size|accum_offset)", l)]
occ = [l.strip() for l in lines[s:e + 200] if "; Occupancy" in l or "; NumVgprs" in l or "; NumSgprs" in l or "; ScratchSize" in l or "; LDSByteSize" in l][:6]

def cls(op):
    if op.startswith("v_pk_"): return "VALU packed fp32 (v_pk_*)"
    if op.startswith(("v_rcp", "v_rsq", "v_sqrt")): return "VALU transcendental"
    if op.startswith(("v_readlane", "v_writelane", "v_readfirstlane")): return "VALU lane<->scalar (incl. SGPR spills)"
    if "_dpp" in op: return "VALU DPP"
    if op.startswith("v_cvt") or "f64" in op: return "VALU f64 / conversions"
    if op.startswith("v_mov"): return "VALU moves"
    if op.startswith("v_"): return "VALU other"
    if op.startswith("ds_"): return "LDS"
    if op.startswith(("global_load_lds",)): return "LDS-DMA"
    if op.startswith(("global_", "scratch_", "buffer_", "flat_")): return "vector memory"
    if op.startswith("s_load"): return "scalar memory"
    if op.startswith("s_waitcnt"): return "s_waitcnt"
    if op.startswith("s_nop"): return "s_nop"
    if op.startswith(("s_cbranch", "s_branch")): return "branches"
    return "SALU other"

print(f"# eu_render5_kernel<3,3,SPHERICAL,FAST,BOXTAB> on top of commit {subprocess.check_output(['git','-C',ROOT,'rev-parse','--short','HEAD']).decode().strip()}{' + working tree' if subprocess.check_output(['git','-C',ROOT,'status','--porcelain','--','envutil_amd/csrc']).strip() else ''} (hipcc -O3 --offload-arch=gfx950 -ffp-contract=off)")
print("## registers of the degree-3 FAST instantiations <NCH,3,SPHERICAL,true,BOXTAB> (before the second loop's groups: 128 VGPRs, 12 / 24 bytes of scratch with the table, 12 / 20 without, occupancy 4)")
for nch in (3, 4):
    for bt in (1, 0):
        k = f"_Z17eu_render5_kernelILi{nch}ELi3ELi0ELb1ELb{bt}EEv"
        ks = next(i for i, l in enumerate(lines) if l.startswith(k))
        info = [l.strip("; ").strip() for l in lines[ks:next(i for i in range(ks, len(lines)) if "; Occupancy" in lines[i]) + 1]
                if re.search(r"; (NumVgprs|ScratchSize|Occupancy):", l)]
        print(f"   <{nch},3,0,true,{'true' if bt else 'false'}>  " + "  ".join(info))
print("## code-object metadata")
for m in meta + occ: print("  ", m)
print("   waves per SIMD by registers: 512 / 128 = 4 (launch bounds 256 x 4); workgroups per CU by LDS: 163840 / 39936 = 4 -> 16 waves per CU")
tot = collections.Counter(cls(op) for _, op in ins)
print(f"## static instruction mix of the whole kernel ({len(ins)} instructions: two loops, one copy of the first loop's body, one of the second's position with its member and pass loops)")
for k, v in tot.most_common(): print(f"   {v:6d}  {k}")
# the first loop's body: the coordinate stage of a group (up to the y reduction, the only DPP block of that loop),
# then the member stage (a loop over the group's members) from its head to its last store
first_dpp = next(i for i, (_, op) in enumerate(ins) if "_dpp" in op)
last_dpp = first_dpp
while "_dpp" in ins[last_dpp + 1][1] or ins[last_dpp + 1][1].startswith("s_nop"): last_dpp += 1
stores = [i for i, (_, op) in enumerate(ins) if op.startswith("global_store")]
dmas = [i for i, (_, op) in enumerate(ins) if op.startswith("global_load_lds")]
dsr = [i for i, (_, op) in enumerate(ins) if op.startswith("ds_read_b128")]
end16 = next(i for i in stores if i > first_dpp and sum(1 for j in stores if first_dpp < j <= i) == 4)
tile_dma = [i for i in dmas if i > first_dpp][:2]
taps0 = next(i for i in dsr if i > tile_dma[-1])
# head of the loop body: walk back from the DPP block to the loop's first table-value use (behind the kernel's prologue)
head = max([i for i, (_, op) in enumerate(ins) if op.startswith("global_load_dword") and i < first_dpp] + [0])
stages = [("coordinate stage, ONCE PER GROUP (table values -> ray y, two latitude chains, md_to_spline, gate, split, y extent: one DPP reduction of two values)", head, last_dpp + 1),
          ("member stage: the group's ballot and lane reads, then per member the x extent from the plan's table, scalar fit / gate tests", last_dpp + 1, tile_dma[0]),
          ("member stage: LDS-DMA issue + y weights of both pairs + window addresses", tile_dma[0], taps0),
          ("member stage: taps of both pairs (32 + 32 ds_read_b128, 2 x 140 packed operations), the next member's column entries / the next leader's table values, stores", taps0, end16 + 1)]
print("## the first loop's body (a group of 16x16 tiles, 256 pixels per wave each), instructions between stage markers [static; the rare")
print("##   branches (work-list exit, unaligned tails of the DMA loop) are inside the ranges, the DMA loop body counts once]")
tsum = collections.Counter()
per_stage = []
for name, a, b in stages:
    c = collections.Counter(cls(op) for _, op in ins[a:b])
    valu = sum(v for k, v in c.items() if k.startswith("VALU"))
    tsum.update(c)
    per_stage.append(valu)
    print(f"   {name}\n      VALU {valu} (packed {c['VALU packed fp32 (v_pk_*)']}, moves {c['VALU moves']}, lane<->scalar {c['VALU lane<->scalar (incl. SGPR spills)']}, DPP {c['VALU DPP']}, f64/cvt {c['VALU f64 / conversions']}, trans {c['VALU transcendental']}), "
          f"SALU {c['SALU other']}, LDS {c['LDS']}, LDS-DMA {c['LDS-DMA']}, vmem {c['vector memory']}, waitcnt {c['s_waitcnt']}, nop {c['s_nop']}, branches {c['branches']}")
coord, member = per_stage[0], sum(per_stage[1:])
print(f"   VALU per tile: a single {coord + member}, in a group of 2 {coord / 2 + member:.0f}, of 4 {coord / 4 + member:.0f}, of 8 {coord / 8 + member:.0f} (880 before the groups)")
# The second loop's position (eu5_tile_bt: the angles once, a member loop behind them, a pass loop inside it), by the
# compiler's own loop annotations: the pass loop is the depth-3 loop that reads 16-byte windows from LDS, its parents are
# the member loop (depth 2) and the position loop (depth 1). Every block names the innermost loop it lies in.
blocks, cur = [], None                 # (first line, label, [annotation lines])
for i, l in enumerate(body):
    m = re.match(r"^(\.LBB\d+_\d+):|^; %bb\.(\d+):", l)
    if m:
        cur = [i, (m.group(1) or "")[2:], [l]]          # ".LBB22_84" is "BB22_84" in the annotations
        blocks.append(cur)
    elif cur is not None and l.lstrip().startswith(";") and "Loop" in l and not re.match(r"^\s+[a-z]", l):
        cur[2].append(l)
parents = {}                           # loop header -> its parent headers
for b in blocks:
    txt = " ".join(b[2])
    if "Loop Header" in txt and b[1]:
        parents[b[1]] = re.findall(r"Parent Loop (BB\d+_\d+)", txt)
def loops_of(b):
    txt = " ".join(b[2])
    if "Loop Header" in txt and b[1]: return parents[b[1]] + [b[1]]
    m = re.search(r"in Loop: Header=(BB\d+_\d+)", txt)
    return parents.get(m.group(1), []) + [m.group(1)] if m else None
spans = []
for k, b in enumerate(blocks):
    ls = loops_of(b)
    if ls is None:      # a block the compiler names but does not annotate (a preheader, a flow block): where the block before it lies
        ls = spans[-1][2] if spans else []
    spans.append((b[0], blocks[k + 1][0] if k + 1 < len(blocks) else len(body), ls))
def has_taps(h):
    return any(re.match(r"^\s+ds_read_b128", body[i]) for a, e, ls in spans if h in ls for i in range(a, e))
deep = [h for h, ps in parents.items() if len(ps) == 2 and has_taps(h)]
if deep:
    pas = deep[-1]
    pos, mem = parents[pas]
    def count(pred):
        c = collections.Counter()
        for a, e, ls in spans:
            if pred(ls):
                c.update(cls(body[i].split()[0]) for i in range(a, e) if re.match(r"^\s+[a-z]", body[i]) and not body[i].strip().startswith("."))
        return c
    def line(name, c):
        valu = sum(v for k, v in c.items() if k.startswith("VALU"))
        print(f"   {name}\n      VALU {valu} (packed {c['VALU packed fp32 (v_pk_*)']}, moves {c['VALU moves']}, lane<->scalar {c['VALU lane<->scalar (incl. SGPR spills)']}, f64/cvt {c['VALU f64 / conversions']}, trans {c['VALU transcendental']}), "
              f"SALU {c['SALU other']}, LDS {c['LDS']}, LDS-DMA {c['LDS-DMA']}, vmem {c['vector memory']}, smem {c['scalar memory']}, waitcnt {c['s_waitcnt']}, branches {c['branches']}")
        return valu
    print(f"## the second loop's position (eu5_tile_bt), by the compiler's loop annotations: position loop {pos}, member loop {mem}, pass loop {pas}")
    print("##   [static; rare branches (work-list append, DMA tails) are inside, a DMA loop's body counts once]")
    v_pos = line("once per POSITION: dequeue, decode, the leader's record and staging, the ANGLES (ray, range test, root, two atan2 chains), the last member's stores, the next leader's table values",
                 count(lambda ls: pos in ls and mem not in ls))
    v_mem = line("per MEMBER, outside its pass loop: entry and record, staging of the first pass, eu5_spline_xy (both md_to_spline halves, gates, x split), y split, weights, in-loop stores",
                 count(lambda ls: mem in ls and pas not in ls))
    v_pas = line("per PASS of a member: the next pass's record, staging of a later pass, window addresses, the wait, taps (32 ds_read_b128, 140 packed operations)",
                 count(lambda ls: pas in ls))
    print(f"   VALU per one-pass tile: a single {v_pos + v_mem + v_pas}, in a position of 2 {v_pos / 2 + v_mem + v_pas:.0f}, of 4 {v_pos / 4 + v_mem + v_pas:.0f}")
    first = min(a for a, e, ls in spans if pos in ls)
    last = max(e for a, e, ls in spans if pos in ls)
    sc = [i for i, l in enumerate(body) if re.match(r"^\s+scratch_", l)]
    inside = [i for i in sc if any(a <= i < e and pos in ls for a, e, ls in spans)]
    print(f"   scratch accesses of the kernel: {len(sc)} (listing lines {sc}); in blocks of the second loop (lines {first}-{last}): {len(inside)}")
else:
    print("## (the second loop's pass loop was not found in the listing)")
# longest dependent chain: the latitude chain (atan2f with x > 0) between the table values and the base position
print("## longest dependent chain per pixel (operations that each need the previous one's result; eu_math2.h):")
print("   ray y 2 | range test 3 | division y/x: rcp + 7 = 8 | table index 3 + LDS round trip | num/den 3 | division 8 | z, w 2 |")
print("   polynomial s1: 11 (s2's 9 run beside it) | s1 + s2, x * (..) 2 | (xs - lo) - x, hi - .. 3 | sign 1 | f64 subtract 3 |")
print("   FMA division by the extent 5 | * total, - .5, - offset 3 | gate 2 | floor, subtract, convert 3  =  ~62 dependent operations,")
print("   ~50 of them packed (8 cycles each from one wave): ~450 cycles; a 16x16 tile runs two such chains side by side (pairs A, B)")
try:
    t = json.load(open(os.path.join(ROOT, "profiles", "traffic.json")))["workloads"]["headline"]
    print("## executed counts (profiles/polar_share_headline_kernel_stats_pmc.txt, the build with the second loop's groups, per launch of eu_render5_kernel; 786 432 16x8-tile equivalents):")
    for l in open(os.path.join(ROOT, "profiles", "polar_share_headline_kernel_stats_pmc.txt")):
        if not l.startswith("new_ "): continue
        if "eu_render5_kernel" in l and any(k in l for k in ("SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_INSTS_LDS", "SQ_ACTIVE_INST_VALU", "SQ_WAVE_CYCLES", "SQ_WAIT_ANY", "SQ_WAIT_INST_ANY", "GRBM_GUI_ACTIVE", "TCP_TOTAL", "SQ_LDS_BANK", "SQ_LDS_IDX")):
            m = re.search(r"(\S+)\s+n=\s*\d+ mean=(\S+)", l)
            v = float(m.group(2))
            print(f"   {m.group(1):32s} {v:14.4g}   per 128 pixels: {v / 786432:9.1f}")
except Exception as ex:
    print("## (no PMC record found:", ex, ")")
