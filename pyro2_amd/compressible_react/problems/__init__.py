__all__ = ["flame", "rt"]
