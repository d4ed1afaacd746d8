"""Compares the gfx950 instruction streams of two builds of the kernels, kernel by kernel: did a change leave the
pre-existing template instantiations as they were?

Build each tree's translation units with --save-temps (the Makefile's flags), e.g. for forest.hip and qring.hip:
    hipcc --offload-arch=gfx950 -std=c++17 -O3 -fPIC -fvisibility=hidden -fvisibility-inlines-hidden -I<tree>/include \
          -ffp-contract=off --save-temps -c forest.hip -o forest.o
then   python tools/isa_diff.py <old_dir> <new_dir> [forest qring ...] [-v]
(dirs = where the *-hip-amdgcn-amd-amdhsa-gfx950.s files are).  Local branch labels are renumbered and the kernel descriptor's
name, section and kernarg_size lines are left out of the comparison (a kernel argument appended at the end changes only those).
A template flag appended with a default (`bool MC = false`) is matched by dropping a trailing `, false` template argument; new
instantiations with `, true` there are counted, not compared; a kernel that became a template for the flag is matched by dropping
`<false>`.  A function whose full name exists in both builds is matched by
that name first, so kernels of the list that did not get the flag in this change are compared as they are.  --exact: both builds have the same template parameters (no appended
flag): functions are matched by their full names.  A translation unit that exists only in <new_dir> is listed as new.
--ops: for every changed kernel, the instruction count of both builds, the opcodes whose counts differ (old -> new) and both
builds' VGPRs, scratch bytes and occupancy (the compiler's resource comments after each function)."""
import collections
import difflib
import re
import subprocess
import sys

FLAGGED = ("direct_kernel", "rowtile_kernel", "qring_kernel", "qwide_kernel",  # kernels that carry the appended flag
           "sparse_kernel", "sparse_top_kernel", "sparse_q_kernel",
           "contribs_kernel", "contribs_spare_kernel", "interactions_kernel", "background_mask_kernel",  # SETS / CAT
           "interventional_kernel", "approx_kernel",
           "oblivious_tile_kernel", "oblivious_direct_kernel", "oblivious_shap_kernel", "oblivious_inter_kernel",
           "oblivious_iv_kernel",  # CAT
           "vector_tile_kernel", "vector_direct_kernel",  # STAGED (the two oblivious walk kernels carry it too)
           "quantize_kernel", "quantize_pair_kernel", "quantize_bucket_pair_kernel", "quantize_multi_kernel")  # COLS


def functions(path):
    out, cur, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\S+):\s*(;.*)?$", line)
        if m:
            cur, body = m.group(1), []
            continue
        if cur and line.startswith(".Lfunc_end"):
            out[cur] = body
            cur = None
            continue
        if cur:
            text = line.split(";")[0].rstrip()
            text = re.sub(r"\.LBB\d+_", ".LBB_", text)
            text = re.sub(r"\.Ltmp\d+", ".Ltmp", text)
            if any(x in text for x in (".amdhsa_kernel ", ".section", ".amdhsa_kernarg_size")):
                continue
            if text.strip() == ".text":  # (a kernel that became a template moves from .text to a section of its own)
                continue
            if text.strip():
                body.append(text)
    return out


def ops_report(path_old, k_old, body_old, path_new, k_new, body_new):
    """--ops: what a changed kernel's two streams differ in, by opcode count and by resources"""
    count = [collections.Counter(re.sub(r"_e(32|64)$", "", t.split()[0])  # (one opcode under either encoding)
                                 for t in b if t[0] in " \t" and not t.strip().startswith(".")) for b in (body_old, body_new)]
    diff = ", ".join(f"{op} {count[0][op]} -> {count[1][op]}" for op in sorted(set(count[0]) | set(count[1])) if count[0][op] != count[1][op])
    res = []
    for path, k in ((path_old, k_old), (path_new, k_new)):
        tail = open(path).read().split(f"\n{k}:")[1]  # the first comments after the label are the function's own
        res.append(" / ".join(re.search(rf"; {f}: (\d+)", tail).group(1) for f in ("NumVgprs", "ScratchSize", "Occupancy")))
    print(f"    instructions {sum(count[0].values())} -> {sum(count[1].values())}; opcode counts that differ: {diff or 'none'}")
    print(f"    VGPRs / scratch bytes / occupancy: {res[0]} -> {res[1]}")


def demangle(names):
    res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return dict(zip(names, res))


def key(name, new, old_names=()):
    base = name.split("(")[0]
    if new and base not in old_names and any(k in base for k in FLAGGED):
        if base.endswith(", false>"):
            return base[: -len(", false>")] + ">"
        if base.endswith(", true>"):
            return None
        if base.endswith("<false>"):  # a kernel that became a template for the flag
            return base[: -len("<false>")].split(" ")[-1]  # (a template's demangled name leads with its return type)
        if base.endswith("<true>"):
            return None
    return base


def main(argv):
    verbose = "-v" in argv
    exact = "--exact" in argv
    ops = "--ops" in argv
    args = [a for a in argv if a not in ("-v", "--exact", "--ops")]
    old_dir, new_dir, units = args[0], args[1], args[2:] or ["forest", "qring"]
    changed = 0
    for unit in units:
        old_path, new_path = (f"{d}/{unit}-hip-amdgcn-amd-amdhsa-gfx950.s" for d in (old_dir, new_dir))
        try:
            old = functions(old_path)
        except FileNotFoundError:
            old = {}
        new = functions(new_path)
        od, nd = demangle(list(old)), demangle(list(new))
        old_by = {key(od[k], False): k for k in old}
        new_by = {}
        for k in new:
            kk = key(nd[k], not exact, old_by)
            if kk is not None:
                new_by[kk] = k
        same = 0
        for name, k in old_by.items():
            if name not in new_by:
                print(f"{unit}: gone: {name}")
                changed += 1
            elif old[k] == new[new_by[name]]:
                same += 1
            else:
                changed += 1
                print(f"{unit}: CHANGED: {name}")
                if ops:
                    ops_report(old_path, k, old[k], new_path, new_by[name], new[new_by[name]])
                if verbose:
                    print("\n".join(list(difflib.unified_diff(old[k], new[new_by[name]], lineterm=""))[:60]))
        added = [n for n in new_by if n not in old_by]
        flagged = 0 if exact else sum(1 for k in new if key(nd[k], True, old_by) is None)
        print(f"{unit}: {same} of {len(old_by)} pre-existing functions identical; new: {added}; new flagged instantiations: {flagged}")
    return 1 if changed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
