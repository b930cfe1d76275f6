"""Driver of mfma_f64_blocks.hip: issue cost of v_mfma_f64_4x4x4_4b_f64 against v_mfma_f64_16x16x4_f64 and the lane maps
of the four-block form.  Builds the probe if its binary is missing, runs it once and prints the output
(profiles/r05_mfma_f64_blocks.txt is a copy of it).

    python tools/probes/mfma_f64_blocks.py [--rounds 5] [--out FILE]
"""
import argparse
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "mfma_f64_blocks.hip")
EXE = os.path.join(HERE, "mfma_f64_blocks")


def build():
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    subprocess.run([hipcc, "-O2", "--offload-arch=gfx950", SRC, "-o", EXE], check=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the probe's output to this file")
    ap.add_argument("--build-only", action="store_true")
    args = ap.parse_args()
    if args.build_only or not os.path.exists(EXE):
        build()
    if args.build_only:
        return 0
    run = subprocess.run([EXE, str(args.rounds)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(run.stdout)
    sys.stdout.write(run.stdout)
    return run.returncode


if __name__ == "__main__":
    sys.exit(main())
