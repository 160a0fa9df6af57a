"""examples/mnistsvm.m as the reference runs it: all ten digits, each with the hinge and the 0-1 loss -- twenty
one-vs-rest classifiers on the same matrix, trained in ONE run (linearsvm_ovr: one read of D per iteration for a
chunk of classes), then the error table of mnistsvm.m:104-117.

    python examples/mnistsvm_ovr.py [train-images train-labels [test-images test-labels [count]]]

With the idx files the images are cropped, scaled and flattened as mnistsvm.m:61-72 does; without them (the image
files are not part of the reference tree) a synthetic matrix of the same shape and sparsity stands in and the table
has its training columns only.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import admm_project_amd as ap  # noqa: E402

argv = sys.argv[1:]
count = int(argv[4]) if len(argv) > 4 else 6000
testD = testlab = None
if len(argv) >= 2:
    D = ap.synth.read_idx3_images(argv[0], count)
    labels = ap.synth.read_idx1_labels(argv[1], count)
    if len(argv) >= 4:
        testD = ap.synth.read_idx3_images(argv[2])
        testlab = ap.synth.read_idx1_labels(argv[3])
else:
    D = ap.synth.mnist_like_problem(seed=1, m=count, n=400)["D"]
    labels = np.random.default_rng(1).integers(0, 10, size=count).astype(np.float64)

# (a third loss, not in the reference: classes = np.repeat(np.arange(10.0), 3) and
#  lossfunction = ["hinge", "01", "logistic"] * 10 add the logistic classifier of every digit, column 3d + 2)
classes = np.repeat(np.arange(10.0), 2)  # column 2d: digit d, hinge; column 2d + 1: digit d, 0-1
res = ap.linearsvm_ovr(D, labels, 0.5, dict(rho=1.0, classes=classes, lossfunction=["hinge", "01"] * 10,
                                            objevals=1))  # mnistsvm.m:42-43, 88-102
print(f"20 classifiers on {D.shape[0]} x {D.shape[1]}: steps {res['steps'].min()}..{res['steps'].max()}, "
      f"loop {res['runtime'] * 1e3:.1f} ms, setup + loop {res['solverruntime'] * 1e3:.1f} ms")


def errors(M, lab):  # mnistsvm.m:97-100: percentage of samples inside the margin or misclassified
    ell = ap.solvers.ovr_label_matrix(lab, classes)
    return np.mean((1.0 - ell * (M @ res["xopt"])) > 0, axis=0) * 100.0


train = errors(D, labels)
test = errors(testD, testlab) if testD is not None else None
print("\nError Percentages:\n")
print("Digit\tHinge (Train)\t0-1 (Train)" + ("\tHinge (Test)\t0-1 (Test)" if test is not None else ""))
for d in range(10):
    row = f"{d}\t{train[2 * d]:2.4f}\t\t{train[2 * d + 1]:2.4f}"
    if test is not None:
        row += f"\t\t{test[2 * d]:2.4f}\t\t{test[2 * d + 1]:2.4f}"
    print(row)
