"""CPU stand-in for the audit methods of recmodel_amd.engine.HipKernels -- TEST INFRASTRUCTURE ONLY: tests/fake_kernels.py's
NumpyKernels plus half_step_audit[_f64] by tests/audit_ref.py, so that AlsEngine.audit's host logic (the two Gramians and their
all-reduce, the indptr windows of the chunks, the all-reduce of the sums, eta) runs on gloo ranks without a GPU."""
import numpy as np

import audit_ref
from fake_kernels import NumpyKernels


class AuditNumpyKernels(NumpyKernels):
    def audit_workspace_bytes(self, n):
        return 16

    def half_step_audit(self, X, Y, f, ld, bias, indptr, indices, values, n, dense, out_sums, out_rows, ws):
        ip = indptr.numpy()[: n + 1]
        sums, rows = audit_ref.half_step_audit(X.numpy()[:n, :f], Y.numpy()[:, :f], bool(bias), ip, indices.numpy(), values.numpy(),
                                               dense.numpy() if dense is not None else None)
        out_sums.numpy()[:] = sums
        if out_rows is not None:
            out_rows.numpy()[:] = rows

    def half_step_audit_f64(self, X, Y, f, bias, indptr, indices, values, n, dense, out_sums, out_rows, ws):
        self.half_step_audit(X, Y, f, f, bias, indptr, indices, values, n, dense, out_sums, out_rows, ws)
