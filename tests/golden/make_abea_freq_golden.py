"""Writes tests/golden/abea_freq_reference.json: the edge batch of tests/abea_freq_cases.py as call-methylation TSV and what the
reference's own meth-freq prints for it.  freq.c is compiled from the reference tree (first argument; else GBX_REFERENCE_DIR,
else /root/reference, as oracle/build_ref.sh looks for it) into a
scratch directory with a two-line main of ours; only the data it read and wrote is kept.

    python tests/golden/make_abea_freq_golden.py [reference root]
"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import abea_freq_cases as K  # noqa: E402

MAIN = "int freq_main(int argc, char **argv);\nint main(int argc, char **argv) { return freq_main(argc, argv); }\n"
CONFIGS = {                                      # name: (TSV version, header kind, meth-freq options)
    "default": (1, 1, []),
    "split": (1, 1, ["-s"]),
    "c0": (1, 1, ["-c", "0"]),
    "c0_split": (1, 1, ["-c", "0", "-s"]),
    "c5": (1, 1, ["-c", "5"]),
    "strand": (2, 1, []),
    "motifs": (1, 2, ["-s"]),
    "strand_motifs": (2, 2, []),
}


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("GBX_REFERENCE_DIR", "/root/reference")
    src = os.path.join(root, "benchmarks", "abea", "src")
    rows = K.edge_rows()
    out = {"inputs": {}, "outputs": {}, "options": {}}
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "main.c"), "w") as f:
            f.write(MAIN)
        exe = os.path.join(tmp, "meth_freq_ref")
        subprocess.run(["gcc", "-O1", "-w", "-I", src, os.path.join(tmp, "main.c"), os.path.join(src, "freq.c"), "-lm", "-o", exe], check=True)
        for name, (version, kind, opts) in CONFIGS.items():
            text = K.to_text(rows, version, kind)
            r = subprocess.run([exe] + opts, input=text, capture_output=True, check=True)
            out["inputs"]["v%d_k%d" % (version, kind)] = text.decode()
            out["outputs"][name] = r.stdout.decode()
            out["options"][name] = dict(version=version, kind=kind, opts=opts)
    with open(os.path.join(HERE, "abea_freq_reference.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
