#!/bin/bash
# Byte-for-byte comparison with the REAL reference, for a box that has what this image lacks:
# a JVM (>= 8) and the reference's own jar.  Nothing here is used by the tests or the product.
#
#   MC_REFERENCE_JAR=/path/to/metacherchant.jar scripts/compare_with_java.sh [n_reads] [k] [extra environment-finder flags...]
#
# Generates the synthetic workload of DESIGN.md section 3.4 (10 x 5 Mb contigs scaled down to n_reads at 30x), writes it
# as FASTA, runs `java -jar $MC_REFERENCE_JAR --tool environment-finder` and the native `metacherchant` on the same
# files with the same flags, and diffs graph.txt, graph.gfa, seqs.fasta and tsvs/* of every output directory.
# A third leg, when MC_PATCHED_JAR names a jar built from the reference with integration/patches/* applied and
# integration/java/gpu/McGpu.java + integration/jni/mcgpu_jni.c built (integration/README.md): the same command with
# MC_GPU_DEVICE=0, i.e. the original Java host over the C ABI, diffed against the other two.
#   MC_REFERENCE_JAR=... scripts/compare_with_java.sh seq-cov [n_reads] [k]
# runs `--tool seq-cov` both ways instead: four bins of n_reads / 4 reads each, the sequences of --read-file a few reads, one shorter
# than k - 1, one of k - 1 bases and a contig; seq_cov.csv is compared byte for byte (the doubles are Double.toString's: a JDK
# before 19 may print a digit more for rare values).
#   MC_REFERENCE_JAR=... scripts/compare_with_java.sh recipient-visualiser [n_reads] [k]
# runs `--tool recipient-visualiser` both ways: n_reads post-FMT reads, the twelve class files cut from them by where a read lies, a
# dozen genes; every comp_<i>.gfa and comp_<i>_seqs.fasta under <output-dir>/after is compared byte for byte, and so is the set of files.
# Exit status 0 = every file identical.  The Java log's timestamps around "Loading file" ... "Hashtable size" ...
# "Finished processing all sequences!" are printed as the reference's phase times on this box's cores.
set -euo pipefail
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
if [ "${1:-}" != "seq-cov" ] && [ "${1:-}" != "recipient-visualiser" ]; then
N=${1:-200000}; K=${2:-31}; shift $(( $# > 2 ? 2 : $# )) || true
EXTRA=("$@")
[ ${#EXTRA[@]} -eq 0 ] && EXTRA=(--coverage 5 --maxkmers 100000 --bothdirs False)
fi
command -v java >/dev/null || { echo "no java on PATH: this script needs a JVM (the graft image has none)"; exit 2; }
[ -f "${MC_REFERENCE_JAR:-}" ] || { echo "set MC_REFERENCE_JAR to the reference's metacherchant.jar"; exit 2; }
CLI="$ROOT/metacherchant_amd/lib/metacherchant"
[ -x "$CLI" ] || python3 -c "import sys; sys.path.insert(0, '$ROOT'); import __graft_entry__ as g; g.build()"
W="$(mktemp -d)"; trap 'rm -rf "$W"' EXIT
if [ "${1:-}" = "seq-cov" ]; then
    N=${2:-200000}; K=${3:-31}
    python3 - "$ROOT" "$W" "$N" "$K" <<'PY'
import sys
root, w, n, k = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
sys.path.insert(0, root)
from oracle import pyoracle as po
L = 150
glen = max(20000, n * L // 30)
genome = po.synth_genome(20240531, glen)
for i, name in enumerate(("donor", "before", "both", "itself")):
    reads = po.synth_reads(genome, 1, glen, 42 + i, 0, n // 4, L, 100)
    with open("%s/%s.fasta" % (w, name), "w") as f:
        for r in range(n // 4):
            f.write(">r%d\n%s\n" % (r, po.decode(reads[r * L:(r + 1) * L])))
q = po.synth_reads(genome, 1, glen, 4242, 0, 1000, L, 100)
with open(w + "/seqs.fasta", "w") as f:
    for r in range(1000):
        f.write(">q%d\n%s\n" % (r, po.decode(q[r * L:(r + 1) * L])))
    f.write(">short\n%s\n>nan\n%s\n>contig\n%s\n" % (po.decode(genome[:k - 2]), po.decode(genome[:k - 1]), po.decode(genome[:glen // 2])))
PY
    BINS=(--from-donor "$W/donor.fasta" --from-before "$W/before.fasta" --from-both "$W/both.fasta" --itself "$W/itself.fasta" -r "$W/seqs.fasta")
    java -jar "$MC_REFERENCE_JAR" --tool seq-cov -k "$K" "${BINS[@]}" -o "$W/java_out" --work-dir "$W/java_wd" --force > "$W/java.stdout" 2> "$W/java.log"
    "$CLI" --tool seq-cov -k "$K" "${BINS[@]}" -o "$W/hip_out" --work-dir "$W/hip_wd" --force 2> "$W/hip.log"
    if cmp -s "$W/java_out/seq_cov.csv" "$W/hip_out/seq_cov.csv"; then echo "identical  seq_cov.csv"; exit 0; fi
    echo "DIFFERENT  seq_cov.csv"; exit 1
fi
if [ "${1:-}" = "recipient-visualiser" ]; then
    N=${2:-20000}; K=${3:-31}
    python3 - "$ROOT" "$W" "$N" "$K" <<'PY'
import os, sys
root, w, n, k = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
sys.path.insert(0, root)
from oracle import pyoracle as po
L = 150
glen = max(20000, n * L // 10)
genome = po.synth_genome(20240531, glen)
reads = po.synth_reads(genome, 1, glen, 42, 0, n, L, 100)
os.makedirs(w + "/classes")
masks = (1, 2, 4, 8, 3, 12, 0, 15)  # by the eighth of the read set a read is in: the classes that get it
names = ("came_from_donor", "came_from_baseline", "came_from_both", "came_itself")
out = {(c, m): open("%s/classes/%s_%s.fasta" % (w, c, m), "w") for c in names for m in "12s"}
with open(w + "/after.fasta", "w") as f:
    for r in range(n):
        s = po.decode(reads[r * L:(r + 1) * L])
        f.write(">r%d\n%s\n" % (r, s))
        for t, c in enumerate(names):
            if masks[r * 8 // n] >> t & 1:
                out[(c, "12s"[r % 3])].write(">r%d\n%s\n" % (r, s))
for f in out.values():
    f.close()
with open(w + "/genes.fasta", "w") as f:
    for g in range(12):
        f.write(">g%d\n%s\n" % (g, po.decode(genome[g * glen // 12:g * glen // 12 + 300])))
    f.write(">absent\n%s\n" % ("ACGT" * 20))
PY
    ARGS=(-k "$K" -after "$W/after.fasta" -seq "$W/genes.fasta" -i "$W/classes" -ext fasta --maxkmers 5000 --maxradius 200)
    java -jar "$MC_REFERENCE_JAR" --tool recipient-visualiser "${ARGS[@]}" -o "$W/java_out" --work-dir "$W/java_wd" --force > "$W/java.stdout" 2> "$W/java.log"
    "$CLI" --tool recipient-visualiser "${ARGS[@]}" -o "$W/hip_out" --work-dir "$W/hip_wd" --force 2> "$W/hip.log"
    status=0
    if [ "$(cd "$W/java_out" && find . -type f | sort)" != "$(cd "$W/hip_out" && find . -type f | sort)" ]; then echo "DIFFERENT  the sets of files"; status=1; fi
    for f in $(cd "$W/java_out" && find . -type f | sort); do
        if cmp -s "$W/java_out/$f" "$W/hip_out/$f"; then echo "identical  $f"; else echo "DIFFERENT  $f"; status=1; fi
    done
    exit $status
fi
python3 - "$ROOT" "$W" "$N" <<'PY'
import sys
root, w, n = sys.argv[1], sys.argv[2], int(sys.argv[3])
sys.path.insert(0, root)
from oracle import pyoracle as po
L = 150
glen = max(20000, n * L // 30)
genome = po.synth_genome(20240531, glen)
reads = po.synth_reads(genome, 1, glen, 42, 0, n, L, 100)
with open(w + "/reads.fasta", "w") as f:
    for i in range(n):
        f.write(">r%d\n%s\n" % (i, po.decode(reads[i * L:(i + 1) * L])))
a = min(10000, glen // 2)
with open(w + "/seed.fasta", "w") as f:
    f.write(">seed\n%s\n" % po.decode(genome[a:a + 500]))
PY
CORES=$(nproc)
t0=$(date +%s.%N)
java -jar "$MC_REFERENCE_JAR" --tool environment-finder -k "$K" --reads "$W/reads.fasta" --seq "$W/seed.fasta" \
     --output "$W/java_out" --work-dir "$W/java_wd" -p "$CORES" --force "${EXTRA[@]}" > "$W/java.stdout" 2> "$W/java.log"
t1=$(date +%s.%N)
"$CLI" --tool environment-finder -k "$K" --reads "$W/reads.fasta" --seq "$W/seed.fasta" \
     --output "$W/hip_out" --work-dir "$W/hip_wd" --force "${EXTRA[@]}" 2> "$W/hip.log"
t2=$(date +%s.%N)
echo "reference (JVM, $CORES cores): $(echo "$t1 - $t0" | bc) s wall; native (MI355X): $(echo "$t2 - $t1" | bc) s wall"
grep -E "Loading file|Hashtable size|Finished processing" "$W/java_wd/log" 2>/dev/null | cut -c1-120 || true
rc=0
while IFS= read -r f; do
    rel="${f#$W/java_out/}"
    if cmp -s "$f" "$W/hip_out/$rel"; then echo "identical  $rel"; else echo "DIFFERENT  $rel"; rc=1; fi
done < <(find "$W/java_out" -type f \( -name graph.txt -o -name graph.gfa -o -name seqs.fasta -o -name '*.tsv' \) | sort)
if [ -f "${MC_PATCHED_JAR:-}" ]; then   # the Java host over the C ABI (integration/: McGpu.java, mcgpu_jni.c, patches)
    MC_GPU_DEVICE=0 java -Djava.library.path="$ROOT/metacherchant_amd/lib" -jar "$MC_PATCHED_JAR" --tool environment-finder -k "$K" \
         --reads "$W/reads.fasta" --seq "$W/seed.fasta" --output "$W/jni_out" --work-dir "$W/jni_wd" -p "$CORES" --force "${EXTRA[@]}" > "$W/jni.stdout" 2> "$W/jni.log"
    while IFS= read -r f; do
        rel="${f#$W/java_out/}"
        if cmp -s "$f" "$W/jni_out/$rel"; then echo "identical (JNI host)  $rel"; else echo "DIFFERENT (JNI host)  $rel"; rc=1; fi
    done < <(find "$W/java_out" -type f \( -name graph.txt -o -name graph.gfa -o -name seqs.fasta -o -name '*.tsv' \) | sort)
fi
[ $rc -eq 0 ] && echo "all output files byte-identical with the reference" || echo "MISMATCH: see above"
exit $rc
