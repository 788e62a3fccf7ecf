from .condition import (  # noqa: F401
    TriangularVectorSolver,
    inverse_norm_estimate,
    triangular_rcond,
    cholesky_rcond,
    cholesky_solve,
)
