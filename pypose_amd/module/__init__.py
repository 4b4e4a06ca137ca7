from .imu_preintegrator import IMUPreintegrator
from .loss import GeodesicLoss, geodesic_loss
from .icp import ICP
from .pnp import EPnP
