from .condition import (  # noqa: F401
    TriangularVectorSolver,
    inverse_norm_estimate,
    triangular_rcond,
    cholesky_rcond,
    cholesky_solve,
)
from .refine import (  # noqa: F401
    HermitianVectorProduct,
    cholesky_info,
    cholesky_refine,
    cholesky_solve_expert,
    cholesky_solve_mixed,
)
