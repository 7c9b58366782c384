from .layer_utils import get_clones, index_points, square_distance

__all__ = ["get_clones", "square_distance", "index_points"]
