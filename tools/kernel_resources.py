"""Register, scratch and LDS use of the instance-minor AP2 kernels, as the compiler reports them.

Compiles awebox_amd/csrc/awegpu.hip for the device only (no GPU needed) with
``-Rpass-analysis=kernel-resource-usage`` and prints, for every ``ap2_soa_*`` kernel, the figures of
the compiler's own remarks (VGPRs, AGPRs, ScratchSize, SGPR / VGPR spills, LDS size, occupancy) and
the kernel's code length, which is the size of its symbol in the code object.  Nothing is derived
from the instruction stream.

    python tools/kernel_resources.py [--label TEXT] [--header FILE] [--kernels REGEX] [--arch gfx950]

``--header`` compiles with another generated node header (``-DAWE_GEN_HEADER``), which is how a
candidate of csrc/gen/ap2_jacgen.cpp is judged before any GPU time is spent on it.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "awebox_amd", "csrc")
FIELDS = ["TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Dynamic Stack", "Occupancy [waves/SIMD]",
          "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]"]


def llvm_tool(hipcc, name):
    for d in (os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "llvm", "bin"),
              os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "lib", "llvm", "bin")):
        if os.path.exists(os.path.join(d, name)):
            return os.path.join(d, name)
    return name


def parse_remarks(text):
    """{mangled name: {field: value}} from the kernel-resource-usage remarks."""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark:\s+(.*?)\s+\[-Rpass-analysis=kernel-resource-usage\]", line)
        if not m:
            continue
        body = m.group(1)
        if body.startswith("Function Name:"):
            cur = out.setdefault(body.split(":", 1)[1].strip(), {})
        elif cur is not None and ":" in body:
            k, v = body.rsplit(":", 1)
            cur[k.strip()] = v.strip()
    return out


def symbol_sizes(readelf, obj):
    """{symbol: bytes} of the FUNC symbols of a code object."""
    r = subprocess.run([readelf, "-sW", obj], check=True, capture_output=True, text=True)
    out = {}
    for line in r.stdout.splitlines():
        f = line.split()
        if len(f) >= 8 and f[3] == "FUNC":
            out[f[7]] = int(f[2], 0)
    return out


def demangle(hipcc, names):
    """Readable kernel names, by whichever demangler is installed (the mangled names otherwise)."""
    import shutil
    for tool in (llvm_tool(hipcc, "llvm-cxxfilt"), "c++filt"):
        if shutil.which(tool):
            out = subprocess.run([tool] + names, capture_output=True, text=True).stdout.splitlines()
            if len(out) == len(names):
                return out
    return names


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--label", default=None, help="heading of the table (default: the header's path)")
    ap.add_argument("--header", default=None, help="generated node header to compile with")
    ap.add_argument("--kernels", default=r"ap2_soa_", help="regular expression on the demangled kernel name")
    ap.add_argument("--arch", default=os.environ.get("AWE_OFFLOAD_ARCH", "gfx950"))
    ap.add_argument("--flags", default="", help="further compiler flags, space separated")
    a = ap.parse_args()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        obj = os.path.join(tmp, "awegpu.co")
        cmd = [hipcc, "-O3", "-std=c++17", f"--offload-arch={a.arch}", "--cuda-device-only", "--no-gpu-bundle-output",
               "-c", "-Rpass-analysis=kernel-resource-usage", "-Wno-unused-value", "-Wno-unused-result", "-I", CSRC]
        if a.header:
            cmd.append('-DAWE_GEN_HEADER="%s"' % os.path.abspath(a.header))
        cmd += a.flags.split() + [os.path.join(CSRC, "awegpu.hip"), "-o", obj]
        r = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            return r.returncode
        res = parse_remarks(r.stderr)
        sizes = symbol_sizes(llvm_tool(hipcc, "llvm-readelf"), obj)
    names = sorted(res)
    dem = demangle(hipcc, names)
    print("== %s" % (a.label or a.header or "awebox_amd/csrc/ap2_nodejac.gen.hpp"))
    print("hipcc -O3 --offload-arch=%s -Rpass-analysis=kernel-resource-usage%s" % (a.arch, " " + a.flags if a.flags else ""))
    for mangled, pretty in zip(names, dem):
        short = re.sub(r"\(.*", "", pretty.replace("(anonymous namespace)::", "")).replace("void ", "")
        if not re.search(a.kernels, short):
            continue
        print("Kernel: %s" % short)
        print("Function Name: %s" % mangled)
        for k in FIELDS:
            print("%s: %s" % (k, res[mangled].get(k, "?")))
        print("Code Length [bytes]: %s" % sizes.get(mangled, "?"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
