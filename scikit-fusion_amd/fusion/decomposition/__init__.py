from .dfmf import Dfmf, DfmfTransform
from .dfmc import Dfmc, DfmcTransform

__all__ = ['Dfmf', 'DfmfTransform', 'Dfmc', 'DfmcTransform']
