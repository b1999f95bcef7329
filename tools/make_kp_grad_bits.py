"""Record tests/golden/kp_grad_bits.json: sha256 digests of what capf_kp_head_backward and capf_kp_heatmap_loss write for the cases of
tests/kp_grad_bits_cases.py, from the library of ONE commit -- the one a later change of the gradient kernels has to reproduce bit for bit.

Needs the MI355X.  Build that commit in a worktree of its own with its own Makefile and point CAPF_LIB at its library:
    CAPF_LIB=<worktree>/contextaware-poseformer_amd/capf/libcapf.so python tools/make_kp_grad_bits.py --commit <hash>     # write the fixture
    python tools/make_kp_grad_bits.py --check                        # the library of this tree against the committed fixture

The file holds the commit's hash, case keys and digests, nothing else; tests/test_gpu_kp_grad_bits.py asserts them."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in ("contextaware-poseformer_amd", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
sys.dont_write_bytecode = True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", help="hash of the commit whose library CAPF_LIB names")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "kp_grad_bits.json"))
    ap.add_argument("--check", action="store_true", help="compare the loaded library with the committed fixture instead of writing one")
    args = ap.parse_args()
    import kp_grad_bits_cases as G
    from capf import lib as capf
    digests = {}
    for group in ("backward", "loss"):
        digests.update(G.compute(group))
    if args.check:
        with open(args.out) as f:
            have = json.load(f)
        assert sorted(have["digests"]) == sorted(digests)
        differ = [k for k in sorted(digests) if have["digests"][k] != digests[k]]
        print(f"{capf.LIB_PATH} against {args.out} (commit {have['commit']}): {len(digests) - len(differ)} of {len(digests)} cases agree")
        for k in differ:
            print("  differs:", k, [o for o in digests[k] if digests[k][o] != have["digests"][k].get(o)])
        sys.exit(1 if differ else 0)
    assert args.commit, "--commit: say which commit's library this is"
    with open(args.out, "w") as f:
        json.dump({"commit": args.commit, "digests": digests}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {args.out}: {len(digests)} cases from {capf.LIB_PATH}, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
