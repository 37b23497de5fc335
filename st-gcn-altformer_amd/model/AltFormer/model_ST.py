"""Drop-in for the reference's ``model/AltFormer/model_ST.py``: ``from model.AltFormer.model_ST import ST`` resolves to the head
whose blocks run on libstgcn_hip.so in inference and on torch ops under autograd (stgcn_amd/altformer.py); no ``timm``, no
``einops``."""
from stgcn_amd.altformer import ST, Attention, Block, DropPath, Mlp  # noqa: F401
