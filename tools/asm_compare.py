"""Device code of two source trees, kernel by kernel: is the set of kernel symbols the same, and is every kernel's instruction text identical?
For refactors that move kernels between units without meaning to change them (profiles/backend_split_ab.txt).  Each csrc/*.hip is compiled with the
Makefile's flags plus -S --cuda-device-only -Rpass-analysis=kernel-resource-usage (cnr_gemm_fdw.hip with its max-ilp strategy); a kernel's text runs
from its label to its .Lfunc_end (the kernel descriptor included), with the function number of the local labels (.LBB<n>_<m> and the BB<n>_<m> of the
loop comments, .Lfunc_end<n>, .Ltmp<n>: a kernel's <n> is its position in its unit) normalised.
The comparison hashes text; the resource columns are the compiler's remarks.  Runs on the CPU box (hipcc cross-compiles).
Usage: python tools/asm_compare.py <parent csrc dir> <new csrc dir>     (a directory that already holds *.s / *.rpass files is taken as it is)"""
import concurrent.futures, glob, hashlib, os, re, subprocess, sys, tempfile

CXXFILT = "/opt/rocm/llvm/bin/llvm-cxxfilt" if os.path.exists("/opt/rocm/llvm/bin/llvm-cxxfilt") else "c++filt"
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wno-unused-function"]


def compile_unit(job):
    f, out = job
    extra = ["-mllvm", "--amdgpu-sched-strategy=max-ilp"] if os.path.basename(f) == "cnr_gemm_fdw.hip" else []
    r = subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + extra + ["-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", f, "-o", out + ".s"],
                       capture_output=True, text=True, cwd=os.path.dirname(f))
    open(out + ".rpass", "w").write(r.stderr)
    return f, r.returncode


def assembly_of(d):
    if glob.glob(os.path.join(d, "*.s")):
        return d
    tmp = tempfile.mkdtemp(prefix="cnr_asm_")
    jobs = [(f, os.path.join(tmp, os.path.basename(f)[:-4])) for f in sorted(glob.glob(os.path.join(d, "*.hip")))]
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        for f, rc in ex.map(compile_unit, jobs):
            if rc != 0:
                sys.exit("compile failed: " + f)
    return tmp


def kernels_of(d):
    """{symbol: [(unit, sha1 of the normalised text, instruction lines, resources)]}"""
    found = {}
    for s in sorted(glob.glob(os.path.join(d, "*.s"))):
        unit = os.path.basename(s)[:-2]
        txt = open(s).read()
        res = {}
        rp = s[:-2] + ".rpass"
        if os.path.exists(rp):
            for m in re.finditer(r"Function Name: (\S+)(.*?)LDS Size \[bytes/block\]: (\d+)", open(rp).read(), re.S):
                g = lambda key: int(re.search(key + r": (\d+)", m.group(2)).group(1))
                res[m.group(1)] = (g(r"VGPRs"), g(r"AGPRs"), g(r"SGPRs"), g(r"ScratchSize \[bytes/lane\]"), int(m.group(3)))
        for name in re.findall(r"^\s*\.amdhsa_kernel (\S+)", txt, re.M):
            m = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:" % re.escape(name), txt, re.S | re.M)
            body = re.sub(r"BB\d+_(\d+)", r"BB_\1", m.group(1))     # labels, and the "Loop: Header=BB<n>_<m>" comments
            body = re.sub(r"\.L(func_end|func_begin|tmp)\d+", r".L\1", body)
            body = re.sub(r"[ \t]+", " ", body)                       # (a label's comment is padded to a column: its width moves with <n>)
            n_ins = sum(1 for l in body.split("\n") if l.startswith(" ") and not l.startswith(" ."))
            found.setdefault(name, []).append((unit, hashlib.sha1(body.encode()).hexdigest(), n_ins, res.get(name)))
    return found


def main():
    old, new = kernels_of(assembly_of(sys.argv[1])), kernels_of(assembly_of(sys.argv[2]))
    twice = [k for k, v in new.items() if len(v) > 1] + [k for k, v in old.items() if len(v) > 1]
    lost, added = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    same = differ = 0
    print("%-18s %-18s %-72s %6s %5s %5s %5s %7s %6s  %s" % ("unit (parent)", "unit (new)", "kernel", "instr", "VGPR", "AGPR", "SGPR", "scratch", "LDS", "text"))
    for k in sorted(set(old) & set(new), key=lambda k: (new[k][0][0], k)):
        (uo, ho, no, ro), (un, hn, nn, rn) = old[k][0], new[k][0]
        ok = ho == hn and ro == rn
        same += ok
        differ += not ok
        d = subprocess.run([CXXFILT, "-p", k], capture_output=True, text=True).stdout.strip()
        r = rn or (-1,) * 5
        print("%-18s %-18s %-72s %6d %5d %5d %5d %7d %6d  %s" % (uo, un, d[:72], nn, r[0], r[1], r[2], r[3], r[4],
                                                                     "identical" if ok else "DIFFERS (parent: %d instr, %s)" % (no, ro)))
    print("kernels: parent %d, new %d; identical %d, differing %d; lost %s; added %s; defined twice %s" % (len(old), len(new), same, differ, lost, added, twice))
    return 0 if not (differ or lost or added or twice) else 1


if __name__ == "__main__":
    sys.exit(main())
