from .trainer import SEQTrainer
from .pseudo import PseudoLabels, pseudo_labels, train_unsupervised
