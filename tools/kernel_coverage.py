#!/usr/bin/env python3
"""Which cache-policy instantiations of the library a kernel trace shows.

    rocprofv3 --kernel-trace --stats -d DIR -o NAME --output-format csv -- python -m pytest tests/test_gpu_cache_policy.py -m gpu
    python tools/kernel_coverage.py matrix-fhe-lattigo_amd/lib/libringhip.so DIR/**/NAME_kernel_trace.csv > profiles/cache_policy_kernel_coverage.txt

    python tools/kernel_coverage.py --multiset DIR/**/NAME_kernel_trace.csv > profiles/ntt_launch_multiset.txt

Lists the kernels of the library's gfx950 code objects (the .hip_fatbin section's offload bundles, symbols with a kernel descriptor) and
counts each one's launches in the trace.  --multiset: the sorted multiset of (kernel, grid, workgroup, LDS bytes) with its count, to compare
the launches of two builds over the same tests.  NT_ARG names, per kernel family, the template argument that selects non-temporal data streams."""
import collections
import csv
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
NT_ARG = {"ntt_fwd_onepass_asm": 1, "ntt_inv_onepass_asm": 1, "ntt_fwd_cols_asm": 1, "ntt_inv_cols_asm": 1, "ntt_fwd_tile_asm": 0,
          "ntt_inv_tile_asm": 0, "ntt_fwd_cols_expand_asm": 1, "ntt_fwd_tile_submul_asm": 1, "ntt_fwd_fused_gap_asm": 2, "ntt3n_layer_asm": 2,
          "ntt_polymul_tile_asm": 0, "ntt_fwd_fused_asm": 2, "ntt_inv_fused_asm": 3, "ntt_ci_fwd_fused_asm": 1, "ntt_ci_inv_fused_asm": 1,
          "ntt_polymul_fused_asm": 1}
PIPELINED = ("ntt_fwd_fused_asm", "ntt_inv_fused_asm", "ntt_ci_fwd_fused_asm", "ntt_ci_inv_fused_asm", "ntt_polymul_fused_asm")
# the row-streaming kernels of csrc/stream_kernels.hip.hpp: non-temporal by a runtime argument
RUNTIME_NT = ("vec_op_packed", "bfv_tensor_kernel", "bgv_tensor_kernel", "bgv_mul_plain_kernel", "bgv_axpby_kernel",
              "ckks_tensor_kernel", "ckks_mul_plain_kernel", "ckks_scalar_kernel", "ckks_scale_then_add_kernel")


def short(name):
    """'void f<1, true>(args)' -> 'f<1, true>'"""
    name = name.strip().strip('"')
    name = re.sub(r"^void ", "", name)
    depth = 0
    for i, ch in enumerate(name):
        depth += ch == "<"
        depth -= ch == ">"
        if ch == "(" and depth == 0:
            return name[:i]
    return re.sub(r"\.kd$", "", name)


def library_kernels(lib):
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    names = set()
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, "fatbin")
        subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, fat])
        d = open(fat, "rb").read()
        pos = d.find(magic)
        while pos >= 0:
            q = pos + len(magic)
            cnt, = struct.unpack_from("<Q", d, q); q += 8
            for _ in range(cnt):
                off, size, tl = struct.unpack_from("<QQQ", d, q); q += 24
                triple = d[q:q + tl].decode(); q += tl
                if "gfx950" in triple and size:
                    co = os.path.join(tmp, "co")
                    open(co, "wb").write(d[pos + off:pos + off + size])
                    for line in subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--symbols", "-W", co]).decode().splitlines():
                        m = re.search(r"\s(\S+)\.kd$", line)
                        if m:
                            names.add(m.group(1))
            pos = d.find(magic, pos + len(magic))
    dem = subprocess.run(["c++filt"], input="\n".join(sorted(names)).encode(), stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()
    return sorted({short(x) for x in dem})


def trace_counts(paths):
    n = collections.Counter()
    for p in paths:
        with open(p, newline="") as f:
            for row in csv.DictReader(f):
                n[short(row.get("Kernel_Name") or row.get("Name") or "")] += 1
    return n


def launch_multiset(paths):
    """Counter of (kernel, grid, workgroup, LDS bytes); grid and workgroup as the trace gives them (one column, or _X/_Y/_Z)"""
    n = collections.Counter()
    for p in paths:
        with open(p, newline="") as f:
            for row in csv.DictReader(f):
                dims = lambda key: "x".join(row[c] for c in sorted(row) if c.startswith(key))
                n[(short(row.get("Kernel_Name") or row.get("Name") or ""), dims("Grid_Size"), dims("Workgroup_Size"), row.get("LDS_Block_Size", ""))] += 1
    return n


def nt_of(kernel):
    fam, _, rest = kernel.partition("<")
    if fam not in NT_ARG or not rest:
        return fam, None
    args = [a.strip() for a in rest.rstrip(">").split(",")]
    return fam, args[NT_ARG[fam]] == "true"


def main():
    if sys.argv[1] == "--multiset":
        for (k, g, w, lds), c in sorted(launch_multiset(sys.argv[2:]).items()):
            print("%-64s grid %-16s workgroup %-10s lds %-7s x %d" % (k, g, w, lds, c))
        return
    lib, traces = sys.argv[1], sys.argv[2:]
    kernels, seen = library_kernels(lib), trace_counts(traces)
    nt = [k for k in kernels if nt_of(k)[1] is True]
    dflt = [k for k in kernels if nt_of(k)[1] is False and nt_of(k)[0] in PIPELINED]
    out = ["kernels in the library's gfx950 code objects: %d; kernels of the library launched in the trace: %d" % (len(kernels), sum(1 for k in kernels if seen[k])), ""]
    out.append("non-temporal instantiations (template argument): %d, in the trace: %d" % (len(nt), sum(1 for k in nt if seen[k])))
    out += ["  %-48s %s" % (k, "launches %d" % seen[k] if seen[k] else "NOT IN THE TRACE") for k in nt]
    out += ["", "default-policy instantiations of the pipelined kernels: %d, in the trace: %d" % (len(dflt), sum(1 for k in dflt if seen[k]))]
    out += ["  %-48s %s" % (k, "launches %d" % seen[k] if seen[k] else "NOT IN THE TRACE") for k in dflt]
    out += ["", "kernels that take the policy as a runtime argument (one code path per value; the tests launch each under nt_streams = 0, 1 and 2):"]
    for k in kernels:
        if k.partition("<")[0] in RUNTIME_NT:
            out.append("  %-48s %s" % (k, "launches %d" % seen[k] if seen[k] else "NOT IN THE TRACE"))
    print("\n".join(out))


if __name__ == "__main__":
    main()
