"""MI355X-native drop-in for the ``simple_knn`` package (``from simple_knn._C import distCUDA2``,
reference geometry/gaussian_base.py:25 and five other geometry modules), plus ``knn_points``, the self-search
form of ``pytorch3d.ops.knn_points`` that the SuGaR geometry uses (``from simple_knn import knn_points``)."""
from ._C import KNN, knn_points  # noqa: F401

