"""What the two heads of this package share in reading configuration dicts and instance bags."""


def strip_scope(cfg, *scopes):
    """a copy of cfg whose 'type' has lost a leading scope ('mmdet.', 'mmrotate.')"""
    cfg = dict(cfg)
    t = str(cfg.get("type"))
    for s in scopes:
        if t.startswith(s):
            t = t[len(s):]
    cfg["type"] = t
    return cfg


def field(obj, *names):
    """the first of `names` that obj (a dict or an object) has"""
    for n in names:
        v = obj.get(n) if isinstance(obj, dict) else getattr(obj, n, None)
        if v is not None:
            return v
    raise AttributeError("none of %s in %r" % (", ".join(names), type(obj).__name__))


def optional(obj, name):
    return obj.get(name) if isinstance(obj, dict) else getattr(obj, name, None)
