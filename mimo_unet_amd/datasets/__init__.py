"""Datasets of the reference with a resident counterpart (mimo/datasets/)."""
