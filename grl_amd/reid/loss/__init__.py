from .oim import oim, OIM, OIMLoss
from .cluster_memory import ClusterMemory, ClusterMemoryLoss
from .proxy_memory import ProxyMemory, ProxyMemoryLoss
from .hybrid_memory import HybridMemory, HybridMemoryLoss
from .soft_memory import SoftClusterMemory, SoftClusterMemoryLoss
from .soft_hybrid_memory import SoftHybridMemory, SoftHybridMemoryLoss
from .soft_proxy_memory import SoftProxyMemory, SoftProxyMemoryLoss
from .soft_triplet import SoftTripletLoss
from .ins_contrast import InstanceContrastLoss
from .pairloss import PairLoss
from .triplet import TripletLoss, TripletLoss_OIM

__all__ = ['oim', 'OIM', 'OIMLoss', 'ClusterMemory', 'ClusterMemoryLoss', 'ProxyMemory', 'ProxyMemoryLoss', 'HybridMemory',
           'HybridMemoryLoss', 'SoftClusterMemory', 'SoftClusterMemoryLoss', 'SoftHybridMemory', 'SoftHybridMemoryLoss',
           'SoftProxyMemory', 'SoftProxyMemoryLoss', 'SoftTripletLoss', 'InstanceContrastLoss', 'PairLoss', 'TripletLoss', 'TripletLoss_OIM']
