"""
Instruction counts of one candidate slot of the WPS tile's events phase, from the device assembly of ftk_kernels.hip
(hipcc --offload-arch=gfx950 -O3 --cuda-device-only -S): the step's instantiation of feat_then_wps_kernel, from the
wave scan of the second unrolled slot's unpack to that of the third (one unpack + one apply, with the slot's guards).

    python tools/wps_slot_counts.py ftk_kernels.s [mangled-name substring]
"""
import re
import sys


def main(path, which="feat_then_wps_kernelILb1ELb1ELb1ELb0ELb1ELb1E"):
    lines = open(path).read().splitlines()
    start = next(i for i, l in enumerate(lines) if l.startswith("_ZN") and which in l and l.rstrip().split(":")[0].endswith("Pl"))
    end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
    body = lines[start:end]
    scans = [i for i, l in enumerate(body) if "row_shr:1 " in l]
    seg = [l.split(";")[0].strip() for l in body[scans[1]:scans[2]]]
    ins = [l.split()[0] for l in seg if l and not l.endswith(":") and not l.startswith(".")]
    vec = [i for i in ins if i.startswith(("v_", "ds_", "global_", "buffer_", "flat_"))]
    wide = [i for i in vec if re.search(r"(i64|u64|b64|_co_|addc|subb)", i)]
    sca = [i for i in ins if i.startswith("s_")]
    print(f"{which}: one slot = {len(ins)} instructions: {len(vec)} vector ({len(wide)} of them 64-bit or carry forms), "
          f"{len(sca)} scalar, {sum(i.startswith('s_cbranch') for i in ins)} branches, "
          f"{sum('saveexec' in i for i in ins)} s_and_saveexec regions, {sum(i.startswith('ds_add') for i in ins)} LDS atomics, "
          f"{sum(i in ('s_nop', 's_waitcnt') for i in ins)} s_nop / s_waitcnt")


if __name__ == "__main__":
    main(*sys.argv[1:])
