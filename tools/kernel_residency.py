"""Which planner kernels can be resident beside two blocks of the headline scatter.

Reads the device assembly of `make -C ska-sdp-continuum-imaging-pipeline_amd/csrc asm` (cip_plan.s,
cip_grid.s, cip_scatter_w8.s: the kernels' `.amdhsa_*` directives and `amdhsa.kernels` metadata; no
instruction is looked at) and prints, per planner kernel, the launcher's block size, the VGPRs, the
allocated VGPRs, the LDS, the scratch and spills, and whether a block fits in what two blocks of
the headline scatter instance leave free on a CU.

Usage: python tools/kernel_residency.py [ASM_DIR] [--check]
  ASM_DIR  default ska-sdp-continuum-imaging-pipeline_amd/csrc/build
  --check  exit 1 unless every serial-chain kernel has no LDS, no scratch and fits
"""
import re
import sys
from pathlib import Path

VGPR_GRANULE = 8  # registers per lane the hardware allocates in
VGPRS_PER_SIMD = 512
LDS_PER_CU = 160 * 1024
# bytes (320 dwords): the compiler's allocation granule for gfx950's 160 KiB. A kernel trace reports the
# headline scatter's LDS_Block_Size as 80,896 B (its 80,664 B rounded up to 512), which would leave 2,048 B
# beside two blocks; the stricter figure is used here, and the serial-chain kernels use no LDS either way.
LDS_GRANULE = 1280
SIMDS = 4

# The headline scatter: scatter_kernel<W = 8, float2, WK_F32, false, 1, false, 1, TX = 64, TY = 64>
# (mangled: the template arguments of the benchmark's 2-D complex64 call on 64-cell work tiles)
SCATTER = ("cip_scatter_w8.s", r"scatter_kernelILi8E15HIP_vector_typeIfLj2EELi1ELb0ELi1ELb0ELi1ELi64ELi64EE")
SCATTER_THREADS = 512
SCATTER_BLOCKS_PER_CU = 2

# (file, mangled-name pattern, threads per block of the launcher, dynamic LDS of the launcher, role)
# role "serial": launched by make_plan between the place pass and the order pass on the 2-D
# dense-row path, a few hundred blocks at the most or a pass nothing else overlaps: it must be
# resident beside the scatter. "bulk": advances as scatter blocks retire (not checked).
PLANNER = [
    ("cip_grid.s", r"23prep_wave_totals_kernelE", 64, 0, "serial"),
    ("cip_grid.s", r"17prep_final_kernelE", 64, 0, "serial"),
    ("cip_plan.s", r"23radix_group_hist_kernelE", 256, 0, "serial"),
    ("cip_plan.s", r"17scan_local_kernelILi0EE", 64, 0, "serial"),
    ("cip_plan.s", r"17scan_local_kernelILi1EE", 64, 0, "serial"),
    ("cip_plan.s", r"17scan_local_kernelILi2EE", 64, 0, "serial"),
    ("cip_plan.s", r"15scan_add_kernelE", 256, 0, "serial"),
    ("cip_plan.s", r"17radix_hist_kernelE", 64, 0, "serial"),
    ("cip_plan.s", r"19tile_offsets_kernelE", 256, 0, "serial"),
    ("cip_plan.s", r"15tile_vis_kernelE", 256, 0, "serial"),
    ("cip_plan.s", r"17dirty_mask_kernelE", 256, 0, "serial"),
    ("cip_plan.s", r"16pack_mask_kernelE", 256, 0, "serial"),
    ("cip_plan.s", r"15row_bits_kernelE", 256, 0, "serial"),
    ("cip_plan.s", r"19chunk_counts_kernelE", 256, 0, "serial"),
    ("cip_plan.s", r"17chunk_emit_kernelE", 256, 0, "serial"),
    ("cip_plan.s", r"13gather_kernelE", 256, 0, "serial"),
    ("cip_plan.s", r"17plan_place_kernelI15HIP_vector_typeIfLj2EELi1ELb1ELi3EE", 256, 0, "bulk"),
    ("cip_plan.s", r"20radix_scatter_kernelE", 256, 0, "bulk"),
    ("cip_grid.s", r"12order_kernelILi0ELb1ELi16EE", 256, 0, "bulk"),
]


def round_up(x, g):
    return (x + g - 1) // g * g


def kernels(path):
    """{mangled name: {vgprs, lds, scratch, vgpr_spills, sgpr_spills, max_threads}} of one .s file."""
    out = {}
    cur = None
    meta = {}
    directive = re.compile(r"^\s+\.amdhsa_(kernel|next_free_vgpr|group_segment_fixed_size|private_segment_fixed_size)\s+(\S+)")
    # kernel-level fields of the amdhsa.kernels metadata (the arguments' fields are indented deeper); they
    # come in alphabetical order, .vgpr_spill_count last
    field = re.compile(r"^(?:    |  - )\.(name|vgpr_spill_count|sgpr_spill_count|max_flat_workgroup_size):\s+(\S+)")
    with open(path, encoding="utf-8", errors="replace") as f:
        for line in f:
            if ".amdhsa_" in line:
                m = directive.match(line)
                if m:
                    key, val = m.groups()
                    if key == "kernel":
                        cur = out.setdefault(val, {})
                    elif cur is not None:
                        cur[{"next_free_vgpr": "vgprs", "group_segment_fixed_size": "lds",
                             "private_segment_fixed_size": "scratch"}[key]] = int(val)
                continue
            if line.startswith("  - ."):
                meta = {}  # the next kernel's entry
            m = field.match(line)
            if not m:
                continue
            meta[m.group(1)] = m.group(2)
            if m.group(1) == "vgpr_spill_count":
                k = out.setdefault(meta["name"], {})
                k["vgpr_spills"] = int(meta["vgpr_spill_count"])
                k["sgpr_spills"] = int(meta["sgpr_spill_count"])
                k["max_threads"] = int(meta["max_flat_workgroup_size"])
    return out


def find(table, pattern, path):
    hits = [n for n in table if re.search(pattern, n)]
    if len(hits) != 1:
        raise SystemExit(f"{path}: {len(hits)} kernels match {pattern!r} (want 1)")
    return hits[0], table[hits[0]]


def short(name):
    # (a template instance's arguments end at "EEv": the function's void return type follows them)
    m = re.match(r"_ZN3cip\d+([a-z0-9_]+_kernel)(?:I(.*?)EEv|E)", name)
    if not m:
        return name
    args = re.findall(r"L[ib](\d+)E|HIP_vector_typeI([fd])Lj2EE", m.group(2) + "E" if m.group(2) else "")
    txt = ", ".join(a or {"f": "float2", "d": "double2"}[v] for a, v in args)
    return m.group(1) + (f"<{txt}>" if txt else "")


def main(argv):
    check = "--check" in argv
    pos = [a for a in argv if not a.startswith("--")]
    root = Path(__file__).resolve().parent.parent
    asm = Path(pos[0]) if pos else root / "ska-sdp-continuum-imaging-pipeline_amd" / "csrc" / "build"
    tables = {}

    def table(fname):
        if fname not in tables:
            tables[fname] = kernels(asm / fname)
        return tables[fname]

    sname, sc = find(table(SCATTER[0]), SCATTER[1], SCATTER[0])
    sc_alloc = round_up(sc["vgprs"], VGPR_GRANULE)
    sc_waves = SCATTER_BLOCKS_PER_CU * SCATTER_THREADS // 64 // SIMDS
    free_vgprs = VGPRS_PER_SIMD - sc_waves * sc_alloc
    free_lds = LDS_PER_CU - SCATTER_BLOCKS_PER_CU * round_up(sc["lds"], LDS_GRANULE)
    print("# Planner kernels beside the headline scatter\n")
    print("Generated by `tools/kernel_residency.py` from the device assembly of `make asm` (gfx950).\n")
    print(f"Headline scatter `{short(sname)}`: {SCATTER_THREADS} threads, {sc['vgprs']} VGPRs "
          f"(allocated {sc_alloc}), {sc['lds']} B of LDS (allocated {round_up(sc['lds'], LDS_GRANULE)} in "
          f"{LDS_GRANULE}-byte granules). {SCATTER_BLOCKS_PER_CU} blocks per CU are {sc_waves} waves per SIMD: "
          f"**{free_vgprs} VGPRs per SIMD and {free_lds} B of LDS stay free.**\n")
    print("A block fits when (its waves per SIMD) x (its allocated VGPRs) <= the free VGPRs and its LDS "
          "(static + the launcher's dynamic, in granules) <= the free LDS. Serial-chain kernels must "
          "also use no LDS at all and no scratch.\n")
    print("| kernel | role | threads | waves/SIMD | VGPRs | allocated | LDS B | scratch B | spills | fits |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    bad = []
    for fname, pat, threads, dyn_lds, role in PLANNER:
        name, k = find(table(fname), pat, fname)
        alloc = round_up(k["vgprs"], VGPR_GRANULE)
        wps = (threads // 64 + SIMDS - 1) // SIMDS
        lds = k["lds"] + dyn_lds
        spills = k.get("vgpr_spills", 0) + k.get("sgpr_spills", 0)
        fits = wps * alloc <= free_vgprs and round_up(lds, LDS_GRANULE) <= free_lds
        ok = fits and lds == 0 and k["scratch"] == 0 and spills == 0 and threads <= k.get("max_threads", threads)
        if role == "serial" and not ok:
            bad.append(short(name))
        print(f"| `{short(name)}` | {role} | {threads} | {wps} | {k['vgprs']} | {alloc} | {lds} | {k['scratch']} | "
              f"{spills} | {'yes' if fits else 'no'} |")
    if bad:
        print(f"\nSerial-chain kernels that cannot be resident beside the scatter: {', '.join(bad)}")
    else:
        print("\nEvery serial-chain kernel fits beside two scatter blocks with no LDS and no scratch.")
    return 1 if check and bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
