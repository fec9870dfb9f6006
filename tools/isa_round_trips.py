"""The memory round trips of a kernel, read from the compiled code (needs hipcc, no GPU).

The pivot loop is bound by latency: what a kernel costs is the number of waits on global memory it makes one after the other, and the
comments of price_kernel, ftran_ratio_fast_kernel and pivot_fused_kernel say how many that should be.  The compiler is free to sink a
load into a branch or to wait early, so the claim is checked on the ISA:

  python tools/isa_round_trips.py 'pivot_fused_kernel<0, 2>'                 listing up to the first barrier
  python tools/isa_round_trips.py --barriers 3 'price_kernel<0, true, 8, false>'
  python tools/isa_round_trips.py --resources [kernel ...]                   VGPRs, SGPRs kept in VGPR lanes (v_writelane) and scratch
  python tools/isa_round_trips.py --asm kernels.s ...                        read an assembly file instead of compiling
  python tools/isa_round_trips.py --define RELP_STAMPS ...                   compile with a macro

The listing keeps, in program order, every global / scalar / scratch load and store, every LDS access, every s_waitcnt and barrier,
and the labels and branches between them (the code is listed as laid out, not as executed: a loop body appears once).  Per segment
between barriers it counts the TRIPS: waits on a vector-memory or scalar-memory load after which the same segment issues further
global loads.  The scalar loads of the kernel arguments (from the kernarg segment pointer, s[0:1] .. s[4:5] on entry) are marked and
do not count.  A kernel name matches when the demangled symbol starts with the given text, blanks ignored.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "relp_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-S"]  # (the Makefile's flags)

KEEP = re.compile(r"^(global_|flat_|buffer_|scratch_|s_load|s_buffer_load|ds_|s_waitcnt|s_barrier|s_cbranch|s_branch|s_endpgm|s_setpc)")
GLOBAL_LOAD = re.compile(r"^(global_load|flat_load|buffer_load|global_atomic\S*\s+v\d)")
RESOURCE = re.compile(r"^;\s*(TotalNumSgprs|NumVgprs|NumAgprs|ScratchSize|Occupancy|LDSByteSize)\s*:\s*(\d+)")


def compile_asm(defines):
    out = tempfile.NamedTemporaryFile(suffix=".s", delete=False).name
    cmd = [HIPCC] + FLAGS + ["-D" + d for d in defines] + [os.path.join(CSRC, "kernels.hip"), "-o", out]
    subprocess.check_call(cmd, cwd=CSRC)
    return out


def demangle(names):
    tool = os.path.join(os.path.dirname(os.path.realpath(HIPCC)), "..", "llvm", "bin", "llvm-cxxfilt")
    if not os.path.exists(tool):
        tool = "c++filt"
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, out))


def kernels_of(path):
    """{mangled name: (body lines, {resource: value})} of every kernel (a symbol with an .amdhsa_kernel descriptor)."""
    lines = open(path).read().split("\n")
    descriptors = {line.split()[1] for line in lines if line.strip().startswith(".amdhsa_kernel ")}
    found, name, body, in_body_of, lanes = {}, None, [], {}, {}
    for line in lines:
        label = re.match(r"^([A-Za-z_][\w$.]*):", line)
        if label and label.group(1) in descriptors:
            name, body = label.group(1), []
            found[name] = (body, {})
            continue
        if name is None:
            continue
        hit = RESOURCE.match(line.strip())
        if hit:  # (the "Kernel info" comments follow the descriptor)
            found[name][1][hit.group(1)] = int(hit.group(2))
        if in_body_of.get(name, True):
            if line.strip().startswith(".amdhsa_kernel"):
                in_body_of[name] = False
            else:
                body.append(line)
                spill = re.match(r"\s*v_writelane_b32 (v\d+), s\d+, (\d+)", line)
                if spill:  # an SGPR kept in a lane of a VGPR
                    lanes.setdefault(name, set()).add(spill.groups())
                    found[name][1]["SGPRSpill"] = len(lanes[name])
    return found


def listing(body, barriers):
    """The kept instructions up to barrier number `barriers`, and the trips of each segment."""
    out, trips, segment_trips = [], 0, []
    pending_wait = None  # index in `out` of a wait on memory that no global load has followed yet
    vector_loads = scalar_loads = 0  # global loads / scalar loads of device memory that no wait has retired yet
    issued = False
    seen = 0
    for raw in body:
        text = raw.split(";")[0].strip()
        if not text:
            continue
        if re.match(r"^\.LBB\w+:", text):
            out.append(text)
            continue
        if text.startswith(".") or not KEEP.match(text):
            continue
        note = ""
        scalar = text.startswith(("s_load", "s_buffer_load"))
        if scalar and re.search(r",\s*s\[0:1\],", text):
            note = "   ; kernel arguments"
        elif GLOBAL_LOAD.match(text) or scalar:
            if pending_wait is not None:
                trips += 1
                out[pending_wait] += "   ; <-- trip %d ends here: loads follow" % trips
                pending_wait = None
            issued = True
            if scalar:
                scalar_loads += 1
            else:
                vector_loads += 1
        elif text.startswith("s_waitcnt"):
            # (LDS and the kernel arguments count in lgkmcnt too: such a wait is a trip only while a scalar load of device memory is out)
            if ("vmcnt" in text and vector_loads) or ("lgkmcnt" in text and scalar_loads):
                pending_wait = len(out)
            if "vmcnt(0)" in text:
                vector_loads = 0
            if "lgkmcnt(0)" in text:
                scalar_loads = 0
        out.append("    " + text + note)
        if text.startswith("s_barrier"):
            seen += 1
            # what is still in flight at the end of a segment is waited for once more: a segment that loads makes one trip more than
            # it has waits followed by loads
            segment_trips.append(trips + (1 if issued else 0))
            out.append("    ---- barrier %d: %d trip(s) in this segment as laid out (branches not taken included)" % (seen, segment_trips[-1]))
            trips, pending_wait, issued = 0, None, False
            if seen >= barriers:
                break
    return out, segment_trips


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("kernel", nargs="*")
    parser.add_argument("--asm")
    parser.add_argument("--define", action="append", default=[])
    parser.add_argument("--barriers", type=int, default=1)
    parser.add_argument("--resources", action="store_true")
    args = parser.parse_args()
    path = args.asm or compile_asm(args.define)
    found = kernels_of(path)
    names = demangle(sorted(found))
    squeeze = lambda s: s.replace(" ", "")
    if args.resources:
        print("%-72s %6s %6s %9s %8s" % ("kernel", "VGPRs", "AGPRs", "SGPRspill", "scratch"))
        for mangled in sorted(found, key=lambda k: names[k]):
            r = found[mangled][1]
            short = re.sub(r"^void relp::", "", names[mangled]).split("(")[0]
            if not args.kernel or any(squeeze(short).startswith(squeeze(k)) for k in args.kernel):
                print("%-72s %6d %6d %9d %8d" % (short, r.get("NumVgprs", -1), r.get("NumAgprs", 0), r.get("SGPRSpill", 0), r.get("ScratchSize", 0)))
        return 0
    status = 0
    for wanted in args.kernel:
        hits = [k for k in found if squeeze(re.sub(r"^void relp::", "", names[k])).startswith(squeeze(wanted))]
        if len(hits) != 1:
            print("%s: %d kernels match" % (wanted, len(hits)), file=sys.stderr)
            status = 1
            continue
        out, trips = listing(found[hits[0]][0], args.barriers)
        r = found[hits[0]][1]
        print("== %s" % names[hits[0]].split("(")[0])
        print("   VGPRs %d, SGPRs kept in VGPR lanes %d, scratch %d B (VGPR spills are part of it); trips per segment as laid out, up to barrier %d: %s" % (
            r.get("NumVgprs", -1), r.get("SGPRSpill", 0), r.get("ScratchSize", 0), args.barriers, trips))
        print("\n".join(out))
    return status


if __name__ == "__main__":
    sys.exit(main())
