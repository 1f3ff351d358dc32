from .oim import oim, OIM, OIMLoss
from .cluster_memory import ClusterMemory, ClusterMemoryLoss
from .pairloss import PairLoss
from .triplet import TripletLoss, TripletLoss_OIM

__all__ = ['oim', 'OIM', 'OIMLoss', 'ClusterMemory', 'ClusterMemoryLoss', 'PairLoss', 'TripletLoss', 'TripletLoss_OIM']
