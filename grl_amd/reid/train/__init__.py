from .trainer import SEQTrainer
from .camera import CameraSEQTrainer
from .pseudo import PseudoLabels, ProxyLabels, pseudo_labels, train_unsupervised
