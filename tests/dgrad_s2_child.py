"""One data gradient of tests/test_hip_dgrad_stride2.py in a process of its own.

MMVQA_DGRAD_S2_DENSE (the dense walk over all KH*KW taps instead of the compact parity classes) is read once per
process, so the dense result is computed here under the environment the parent test gives.
Usage: dgrad_s2_child.py CASE.pt OUT.pt -- CASE.pt = {"cfg": (N, H, W, Cin, Cout, K, stride, pad), "G", "w", "tile"},
OUT.pt = {"dx": the [pixel][Cin] result on the CPU}."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for path in (HERE, os.path.dirname(HERE)):
    if path not in sys.path:
        sys.path.insert(0, path)

import torch  # noqa: E402

from hip_helpers import L, conv_desc_dgrad, dev, nhwc, run_igemm, w_ohwi  # noqa: E402


def main(case_path, out_path):
    c = torch.load(case_path)
    N, H, W, Cin, Cout, K, s, p = c["cfg"]
    Gd, wd = nhwc(c["G"]), w_ohwi(c["w"])
    dx = torch.full((N * H * W, Cin), float("nan"), device=dev())
    d = conv_desc_dgrad(Gd, wd, N, H, W, Cin, Cout, K, s, p, dx)
    run_igemm(d, L.KIND_DGRAD, tile=c["tile"])
    torch.save({"dx": dx.cpu()}, out_path)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
