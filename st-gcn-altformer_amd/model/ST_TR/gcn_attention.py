"""Drop-in for ``model/ST_TR/gcn_attention.py`` of the reference: ``from model.ST_TR.gcn_attention import
gcn_unit_attention`` (model/ST_TR/ST_TR_new.py:6, ST_GCN_Trans.py:7).

(``model/ST_TR`` deliberately has no ``__init__.py``: with this directory first on ``sys.path`` the namespace packages
merge, so ``model.ST_TR.gcn_attention`` resolves here and the reference's other ST_TR files still resolve to its own.)
"""
from stgcn_amd.st_attention import gcn_unit_attention  # noqa: F401
