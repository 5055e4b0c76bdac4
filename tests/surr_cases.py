"""Case module beside tests/surr64.py: the surrogate engine's gradient cases and the ratios its test records."""
from tests import surr64 as S


TILE_NS = (1, 15, 17, 65)        # 16-row tiles: a lone row, a tile minus one, a tile plus one, several tiles and a ragged one
CASES = [(H, i, E, L, n) for (H, i, E) in S.SHAPES for L in (1, 2, 4) for n in TILE_NS]


RATIOS = {}
