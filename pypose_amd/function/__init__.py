from .geometry import cart2homo, homo2cart, point2pixel, pixel2point, reprojerr, svdtf, svdstf, bal_point2pixel, bal_reprojerr, knn, \
    nbr_filter, random_filter, voxel_filter, knn_filter, knn_index, KnnIndex
from .checking import is_lietensor, is_SE3, hasnan
from .spline import chspline, bspline
from .linalg import bvv, bmv, bvmv
