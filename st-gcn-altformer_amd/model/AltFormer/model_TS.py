"""Drop-in for the reference's ``model/AltFormer/model_TS.py``: ``from model.AltFormer.model_TS import TS`` resolves to the head
whose blocks run on libstgcn_hip.so in inference and on torch ops under autograd (stgcn_amd/altformer.py); no ``timm``, no
``einops``."""
from stgcn_amd.altformer import TS, Attention, Block, DropPath, Mlp  # noqa: F401
