"""Drop-in for ``model/ST_Vit/trans.py`` of the reference: ``from model.ST_Vit.trans import ViT`` (ST_GCN_Trans.py:9).

(``model/ST_Vit`` deliberately has no ``__init__.py``: with this directory first on ``sys.path`` the namespace packages
merge, so ``model.ST_Vit.trans`` resolves here and the reference's ``ST_GCN_Trans.py`` still resolves to its own file, and
builds its ``ViT`` from this one unedited.  ``einops`` is not needed.)
"""
from stgcn_amd.vit import Attention, FeedForward, PreNorm, Transformer, ViT  # noqa: F401
