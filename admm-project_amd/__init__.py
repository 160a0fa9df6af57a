"""admm-project_amd: MI355X-native ADMM iteration engine behind the admm()/getproxops() surface.

Host side (Python) mirrors the reference's MATLAB interface for the hot path only; all
per-iteration arithmetic runs in hand-written HIP kernels (csrc/) behind a plain C ABI
(include/admm_engine.h -> libadmm_hip.so).  No CPU fallback exists.
"""
from . import _lib, errorcheck, synth  # noqa: F401
from ._lib import AdmmError  # noqa: F401
from .api import ProxOp, admm, getproxops  # noqa: F401
from .engine import Engine, SvmOvr  # noqa: F401
from .reg_multi import RegMulti  # noqa: F401
from .sparse_svm import SparseSvmOvr  # noqa: F401
from .sparse_reg import SparseRegMulti  # noqa: F401
from .sparse_lasso import SparseLassoMulti  # noqa: F401
from .lasso_multi import LassoMulti  # noqa: F401
from .covsel_multi import CovselMulti  # noqa: F401
from .l1class import L1Classifier  # noqa: F401
from .sparse_l1class import SparseL1Classifier  # noqa: F401
from . import testers  # noqa: F401,E402
from .softmax import multinomial, multinomial_lambda_max, multinomial_path, multinomial_proba  # noqa: F401,E402
from .solvers import (basispursuit, covarianceselection, covarianceselection_lambda_max, covarianceselection_multi, covarianceselection_path, elasticnet, grouplasso, grouplasso_multi, grouplasso_path, groupclassifier, groupclassifier_cv, groupclassifier_lambda_max, groupclassifier_multi, groupclassifier_path, huberfit, l1classifier, l1classifier_lambda_max, l1classifier_multi, l1classifier_path, l1classifier_cv, lad, lasso, lasso_cv, lasso_multi, cv_folds, cv_summary, lasso_multi_dense, lasso_path, lasso_path_dense, linearprogram, linearsvm, linearsvm_ovr, model,  # noqa: F401
                      quantilereg, quantilereg_multi, quadraticprogram, robustfit_multi, totalvariation, totalvariation2d, unwrappedadmm)

__version__ = "0.1.0"
