class DISK(object):
    def __init__(self, *a, **k):
        raise NotImplementedError("the stand-in has no DISK")
