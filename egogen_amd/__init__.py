def __getattr__(name):      # `from egogen_amd import GeodesicField` without importing torch with the package
    if name == "GeodesicField":
        from .geodesic import GeodesicField
        return GeodesicField
    if name == "MovingObstacles":
        from .obstacles import MovingObstacles
        return MovingObstacles
    if name == "PersonGroups":
        from .crowd import PersonGroups
        return PersonGroups
    if name == "PolicyProposal":
        from .proposal import PolicyProposal
        return PolicyProposal
    if name == "MotionSet":
        from .metrics import MotionSet
        return MotionSet
    if name == "Routes":
        from .route import Routes
        return Routes
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
